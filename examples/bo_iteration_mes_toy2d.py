#!/usr/bin/env python3
"""One iteration of the max-value entropy search (MES) baseline on the toy 2-D problem of bo_iteration_toy2d.py (2 objectives, 1
constraint, 2 fidelities), every stage on the GPU:

  fit the three exact GPs (``MFGP.fit(engine="device")``)  ->  sample a Pareto front of their posterior function samples
  (``util.mes_front.sample_pareto_front``: the draws of csrc/exact_sample.hip, MOOP on the chain samples)  ->  maximise the
  cost-weighted MES acquisition per fidelity (``MESMOC_MFGP(search="device")``, costs 1 and 10)  ->  next (x, fidelity).

MES maximises: the objective models are fitted to the NEGATED observations of the minimised black-boxes; the constraint is
feasible when >= 0.

    python examples/bo_iteration_mes_toy2d.py [--fit-iters 200] [--features 500] [--seed 0]
"""
import argparse
import faulthandler
import os
import sys
import time

import numpy as np

faulthandler.enable()      # a native crash leaves the Python stack on stderr
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bo_iteration_toy2d import blackboxes  # noqa: E402
from mobocmf_amd.acquisition_functions.MESMOC_MFGP import MESMOC_MFGP  # noqa: E402
from mobocmf_amd.models.mfgp import MFGP  # noqa: E402
from mobocmf_amd.util.mes_front import sample_pareto_front  # noqa: E402


def run(fit_iters=200, nFeatures=500, acq_iters=50, n_low=14, n_high=6, grid=1000, seed=0, device="cuda", verbose=True, data=None,
        fit_engine="device", sample_engine="device", acq_search="device", refine="device", pareto_search="grid", **moop_kwargs):
    """Returns (models, front, acq, candidate, fidelity, seconds) -- ``front`` the ``SampledFront``, ``seconds`` the
    fit / sample / search split."""
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    if data is None:
        x = rng.uniform(size=(n_low + n_high, 2))
        fid = np.concatenate([np.zeros(n_low), np.ones(n_high)])
    else:
        x, fid = data
    xt = torch.from_numpy(np.concatenate([x, fid[:, None]], 1))
    objectives, constraints = {}, {}
    for name, (lo, hi, is_con) in blackboxes().items():
        y = np.where(fid == 0, lo(x), hi(x))
        model = MFGP(xt, torch.from_numpy(y if is_con else -y), 2).to(device)
        (constraints if is_con else objectives)[name] = model
    sync = torch.cuda.synchronize if torch.device(device).type == "cuda" else (lambda: None)
    t = [time.perf_counter()]
    for model in list(objectives.values()) + list(constraints.values()):
        model.fit(num_iters=fit_iters, engine=fit_engine)
    sync(); t.append(time.perf_counter())
    thresholds = {name: 0.0 for name in constraints}
    gen = torch.Generator(device=device).manual_seed(seed)
    front = sample_pareto_front(objectives, constraints, thresholds, x, 2, nFeatures=nFeatures, generator=gen, rng=rng,
                                engine=sample_engine, grid_size=grid, refine=refine, search=pareto_search, **moop_kwargs)
    sync(); t.append(time.perf_counter())
    bounds = torch.tensor([[0.0, 0.0], [1.0, 1.0]], dtype=torch.float64, device=device)
    acq = MESMOC_MFGP(objectives, constraints, 2, 2, front.best_objective_values, thresholds, standard_bounds=bounds,
                      search=acq_search)
    for f in range(2):
        for name, (_, _, is_con) in blackboxes().items():
            acq.add_blackbox(f, name, cost_evaluation=1.0 if f == 0 else 10.0, is_constraint=is_con)
    cand, fidelity = acq.get_nextpoint_coupled(iteration=0, verbose=verbose, maxiter=acq_iters, generator=gen)
    sync(); t.append(time.perf_counter())
    seconds = tuple(b - a for a, b in zip(t[:-1], t[1:]))
    if verbose:
        print("sampled front %s after %d constraint draw(s), engines %s" % (tuple(front.pareto_front.shape), front.tries, front.engines))
        print("best objective values", front.best_objective_values)
        print("seconds: fit %.3f | sample %.3f | search %.3f" % seconds)
        print("next point", cand.cpu().numpy(), "at fidelity", fidelity)
    return dict(objectives=objectives, constraints=constraints), front, acq, cand, fidelity, seconds


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--fit-iters", type=int, default=200)
    ap.add_argument("--features", type=int, default=500)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--pareto-search", choices=["grid", "evolve"], default="grid")
    a = ap.parse_args()
    run(fit_iters=a.fit_iters, nFeatures=a.features, seed=a.seed, pareto_search=a.pareto_search)
