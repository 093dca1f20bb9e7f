#!/usr/bin/env python3
"""The BO loop of bo_loop_hv_toy2d.py with DECOUPLED evaluations: every black-box keeps its own data set, each iteration asks
which black-box to evaluate next, where and at which fidelity (``JESMOC_MFDGP.get_nextpoint_decoupled``: every black-box's own
JES term maximised and weighed by that black-box's evaluation cost), and ONLY the chosen black-box is evaluated there.  The
recommendation is scored as in bo_loop_hv_toy2d.py and appended to ``hypervolumes.txt`` in the same six columns.

``--acq random``: the baseline, a uniformly chosen (fidelity, black-box) and a uniform point
(``Random_choice.get_nextpoint_decoupled``).  ``--search device`` keeps the searches of all black-boxes of a fidelity on the GPU
(util/acq_search.py DecoupledDeviceAcqSearch).  ``--pareto-samples K`` averages JES over K sampled Pareto sets.

    python examples/bo_loop_decoupled_toy2d.py [--iters 5] [--acq jes|random] [--search host|device] [--pareto-samples K]
                                               [--epochs 300] [--seed 0] [--out .]
"""
import argparse
import faulthandler
import os
import sys
import time

import numpy as np

faulthandler.enable()
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bo_iteration_toy2d import blackboxes  # noqa: E402
from bo_loop_hv_toy2d import score  # noqa: E402
from mobocmf_amd.acquisition_functions.JESMOC_MFDGP import JESMOC_MFDGP  # noqa: E402
from mobocmf_amd.acquisition_functions.Random_choice import Random_choice  # noqa: E402
from mobocmf_amd.models.mfdgp import TL  # noqa: E402
from mobocmf_amd.util.blackbox_mfdgp_fitter import BlackBoxMFDGPFitter  # noqa: E402

COSTS = (1.0, 10.0)      # the cost of one evaluation of one black-box at fidelity 0 / 1


def fit(data, epochs, seed, device="cuda", grid=100):
    """The unconditioned fit of every black-box on ITS OWN rows: ``data``: name -> (x (n, 2), fid (n,))."""
    torch.manual_seed(seed)
    np.random.seed(seed)
    fitter = BlackBoxMFDGPFitter(2, max(x.shape[0] for x, _ in data.values()), num_epochs_1=epochs, num_epochs_2=epochs,
                                 pareto_set_size=10, opt_grid_size=grid, type_lengthscale=TL.MEDIAN, device=device,
                                 decoupled_evals=True)
    fitter.verbose = False
    for name, (lo, hi, is_con) in blackboxes().items():
        x, fid = data[name]
        y = np.where(fid == 0, lo(x), hi(x))
        fitter.initialize_mfdgp(torch.from_numpy(x), torch.from_numpy(y)[:, None], torch.from_numpy(fid)[:, None], name,
                                is_constraint=is_con)
    fitter.train_mfdgps()
    return fitter


def choose(fitter, search="host", pareto_samples=1, cond_iters=200, acq_iters=50, device="cuda", iteration=None, verbose=False):
    """Pareto sample(s), conditioned fit(s), the decoupled search: (acquisition, x, fidelity, name, is_constraint)."""
    fitter.sample_and_store_pareto_solution()
    fitter.num_epochs_2 = cond_iters
    acq = JESMOC_MFDGP(model=fitter, num_fidelities=2, search=search, num_pareto_samples=pareto_samples,
                       standard_bounds=torch.tensor([[0.0, 0.0], [1.0, 1.0]], dtype=torch.float64, device=device))
    for f in range(2):
        for name, (_, _, is_con) in blackboxes().items():
            acq.add_blackbox(f, name, cost_evaluation=COSTS[f], is_constraint=is_con)
    return (acq,) + tuple(acq.get_nextpoint_decoupled(iteration=iteration, verbose=verbose, maxiter=acq_iters))


def loop_decoupled(iters=5, acq="jes", seed=0, out_dir=".", epochs=300, verbose=True, search="host", pareto_samples=1, **kw):
    """``iters`` iterations, each one scored and appended to ``out_dir``/hypervolumes.txt; returns (rows, choices, data)."""
    rng = np.random.default_rng(seed)
    x0 = rng.uniform(size=(20, 2))
    fid0 = np.concatenate([np.zeros(14), np.ones(6)])
    data = {name: (x0.copy(), fid0.copy()) for name in blackboxes()}
    grid = np.random.default_rng((seed, 1000)).uniform(size=(1000 * 2, 2))
    chooser = None
    if acq == "random":
        chooser = Random_choice(input_size=2, num_fidelities=2, seed=seed)
        for f in range(2):
            for name, (_, _, is_con) in blackboxes().items():
                chooser.add_blackbox(f, name, cost_evaluation=COSTS[f], is_constraint=is_con)
    rows, choices = [], []
    path = os.path.join(out_dir, "hypervolumes.txt")
    for it in range(iters):
        t0 = time.perf_counter()
        fitter = fit(data, epochs, seed + it)
        row = score(fitter, grid)      # (before the search: the conditioned fit of sample 0 trains this fitter's own models)
        with open(path, "a") as f:
            print("%lf %lf %lf %lf %lf %lf" % row, file=f)
        rows.append(row)
        if acq == "random":
            cand, fidelity, name, is_con = chooser.get_nextpoint_decoupled(iteration=it)
        else:
            _, cand, fidelity, name, is_con = choose(fitter, search=search, pareto_samples=pareto_samples, iteration=it, **kw)
        x, fid = data[name]            # only the chosen black-box is evaluated
        data[name] = (np.vstack([x, cand.detach().cpu().numpy().reshape(1, -1)]), np.concatenate([fid, [float(fidelity)]]))
        choices.append((name, int(fidelity), bool(is_con)))
        if verbose:
            print("Iter: %d  evaluate %s at fidelity %d  HV recommendation %.6f  optimal %.6f  feasible %d  points %d/%d  (%.1f s)"
                  % (it, name, fidelity, row[0], row[1], row[2], row[4], row[5], time.perf_counter() - t0))
    return rows, choices, data


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--acq", choices=["jes", "random"], default="jes")
    ap.add_argument("--search", choices=["host", "device"], default="host", help="where the acquisition search runs")
    ap.add_argument("--pareto-samples", type=int, default=1,
                    help="average the JES acquisition over this many sampled Pareto sets (one conditioned fit each)")
    ap.add_argument("--epochs", type=int, default=300)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=".")
    a = ap.parse_args()
    loop_decoupled(iters=a.iters, acq=a.acq, seed=a.seed, out_dir=a.out, epochs=a.epochs, search=a.search,
                   pareto_samples=a.pareto_samples)
