#!/usr/bin/env python3
"""The reference's BO loop with its score (toy_synthetic_2D_JESMOCMF.py:533-627) on the toy 2-D problem of
bo_iteration_toy2d.py: after every iteration the fitted models recommend a Pareto set on a fixed seeded grid of 1000 d points
(``BlackBoxMFDGPFitter.recommend``), and its true hypervolume, the true optimum's on the same grid and the counts are appended
to ``hypervolumes.txt`` in the reference's six columns:

    hv_iter  optimal_hv  feasible  num_infeasible  num_optimal_points_fini  num_optimal_points_ini

``--acq jes`` (default) chooses the next point with bo_iteration_toy2d.run (the cost-weighted JES acquisition), ``--acq random``
with the reference's random baseline (Random_choice), ``--acq mes`` with the max-value entropy search baseline on exact GPs
(bo_iteration_mes_toy2d.run: device fit, sampled Pareto front, device acquisition search).  Objectives are minimised, the
constraint is feasible when >= 0; the reference point of the hypervolume is (1000, 1000), as there.

With ``--acq mes`` the row that is scored comes from ``fit_only``'s MFDGP recommendation on the data the acquisition has
gathered, as for ``--acq random`` (the exact GPs only choose the next point).  All three acquisitions are thus scored by the same
recommender, the MFDGP surrogates' ``recommend``, and the columns compare acquisitions, not models.

``--num-inducing M`` caps the inducing points of every surrogate at M; ``--inducing greedy`` then chooses them among the
training rows by greedy conditional variance (``inducing_selection="greedy_variance"``) instead of taking the first M rows.

``--warm-start`` starts every iteration after the first from the previous iteration's unconditioned fit
(``warm_start="posterior"``) and trains ``--warm-epochs`` epochs of phase 2 only (default: ``--epochs``).  The new inducing
inputs must extend the old ones, which all training rows and the first M rows do and a greedy re-selection in general does not.

``--pareto-samples K`` averages the JES acquisition over K sampled Pareto sets (JESMOC_MFDGP(num_pareto_samples=K)).

    python examples/bo_loop_hv_toy2d.py [--iters 5] [--acq jes|random|mes] [--epochs 300] [--seed 0] [--out .]
                                        [--num-inducing M] [--inducing first|greedy] [--warm-start [--warm-epochs E]]
                                        [--pareto-samples K]
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
from bo_iteration_mes_toy2d import run as mes_run  # noqa: E402
from bo_iteration_toy2d import blackboxes, run  # noqa: E402
from mobocmf_amd.acquisition_functions.Random_choice import Random_choice  # noqa: E402
from mobocmf_amd.models.mfdgp import TL  # noqa: E402
from mobocmf_amd.util.blackbox_mfdgp_fitter import BlackBoxMFDGPFitter  # noqa: E402
from mobocmf_amd.util.hypervolume import HV  # noqa: E402
from mobocmf_amd.util.moop import MOOP  # noqa: E402

REF_POINT = np.array([1000.0, 1000.0])


def fit_only(x, fid, epochs, seed, device="cuda", model_kwargs=None, previous=None, warm_epochs=None):
    """The unconditioned fit of bo_iteration_toy2d.run alone: what the random baseline recommends from."""
    torch.manual_seed(seed)
    warm = previous is not None and warm_epochs is not None
    fitter = BlackBoxMFDGPFitter(2, x.shape[0], num_epochs_1=0 if warm else epochs,
                                 num_epochs_2=warm_epochs if warm else epochs, type_lengthscale=TL.MEDIAN, device=device,
                                 **(model_kwargs or {}))
    fitter.verbose = False
    for name, (lo, hi, is_con) in blackboxes().items():
        y = np.where(fid == 0, lo(x), hi(x))
        start = {}
        if warm:
            start = dict(previously_trained_model=previous.get_model(name, is_constraint=is_con), warm_start="posterior")
        fitter.initialize_mfdgp(torch.from_numpy(x), torch.from_numpy(y)[:, None], torch.from_numpy(fid)[:, None], name,
                                is_constraint=is_con, **start)
    fitter.train_mfdgps()
    return fitter


def score(fitter, grid, recommend_search="grid"):
    """The six numbers of one iteration (toy_synthetic_2D_JESMOCMF.py:537-618) on the true high-fidelity functions.
    ``recommend_search``: ``recommend``'s ``search`` ("evolve": NSGA-II on the GPU over the predictions, from the grid's rows)."""
    bb = blackboxes()
    objs = [hi for _, hi, is_con in bb.values() if not is_con]
    cons = [hi for _, hi, is_con in bb.values() if is_con]
    ind = HV(ref_point=REF_POINT)
    rec_set, _, _ = fitter.recommend(grid, min_feasible_prob=0.999, search=recommend_search)
    true_cons = np.stack([c(rec_set) for c in cons], 1) if rec_set.shape[0] else np.zeros((0, len(cons)))
    feasible = not np.any(true_cons < 0)
    num_ini = rec_set.shape[0]
    rec_set = rec_set[np.all(true_cons >= 0, axis=1)]
    num_fini = rec_set.shape[0]
    hv_iter = ind(np.stack([f(rec_set) for f in objs], 1)) if num_fini else 0.0
    ok = np.all(np.stack([c(grid) for c in cons], 1) > 0, axis=1)
    feas_objs = np.stack([f(grid) for f in objs], 1)[ok]
    optimal_hv = ind(feas_objs[MOOP.compute_pareto_front(feas_objs)]) if feas_objs.shape[0] else 0.0
    return hv_iter, optimal_hv, float(feasible), num_ini - num_fini, num_fini, num_ini


def loop_hv(iters=5, acq="jes", seed=0, out_dir=".", epochs=300, verbose=True, num_inducing=None, inducing="first",
            warm_start=False, warm_epochs=None, pareto_samples=1, pareto_search="grid", recommend_search="grid", record=None,
            **kw):
    """``iters`` BO iterations, each one scored and appended to ``out_dir``/hypervolumes.txt; returns the rows.
    ``warm_start``: every iteration after the first starts from the last one's unconditioned fit, ``warm_epochs`` epochs of
    phase 2 (default: ``epochs``).  ``pareto_samples``: JES averaged over this many sampled Pareto sets.  ``pareto_search``: the fitter's
    (``"evolve"``: NSGA-II on the GPU from the grid's rows).  ``recommend_search``: how the recommendation that is scored is
    searched (``score``).  ``acq="mes"``: ``kw`` goes to bo_iteration_mes_toy2d.run; ``record``: a list that receives, per
    iteration, dict(rows, search_engine, sample_engines, tries) of the MES iteration."""
    warm_epochs = (epochs if warm_epochs is None else warm_epochs) if warm_start else None
    previous = None
    model_kwargs = {"pareto_search": pareto_search}
    if num_inducing is not None:
        model_kwargs.update(num_inducing=num_inducing,
                            inducing_selection="greedy_variance" if inducing == "greedy" else "first")
    rng = np.random.default_rng(seed)
    x = rng.uniform(size=(20, 2))
    fid = np.concatenate([np.zeros(14), np.ones(6)])
    grid = np.random.default_rng((seed, 1000)).uniform(size=(1000 * 2, 2))
    chooser = None
    if acq == "random":
        chooser = Random_choice(input_size=2, num_fidelities=2, seed=seed)
        for f in range(2):
            for name in blackboxes():
                chooser.add_blackbox(f, name, cost_evaluation=1.0 if f == 0 else 10.0)
    rows = []
    path = os.path.join(out_dir, "hypervolumes.txt")
    for it in range(iters):
        t0 = time.perf_counter()
        if acq == "random":
            fitter = fit_only(x, fid, epochs, seed + it, model_kwargs=model_kwargs, previous=previous,
                              warm_epochs=warm_epochs)
            previous = fitter if warm_start else None
            cand, fidelity = chooser.get_nextpoint_coupled(iteration=it)
        elif acq == "mes":
            fitter = fit_only(x, fid, epochs, seed + it, model_kwargs=model_kwargs, previous=previous,
                              warm_epochs=warm_epochs)
            previous = fitter if warm_start else None
            _, front, mes, cand, fidelity, _ = mes_run(seed=seed + it, data=(x, fid), verbose=False, **kw)
            if record is not None:
                record.append(dict(rows=x.shape[0], search_engine=dict(mes.last_search_engine),
                                   sample_engines=dict(front.engines), tries=front.tries))
        else:
            fitter, jes, cand, fidelity = run(seed=seed + it, data=(x, fid), epochs=epochs, verbose=False,
                                              model_kwargs=model_kwargs, previous=previous, warm_epochs=warm_epochs,
                                              pareto_samples=pareto_samples, **kw)
            previous = jes.blackbox_mfdgp_fitter_uncond if warm_start else None
        row = score(fitter, grid, recommend_search)
        with open(path, "a") as f:
            print("%lf %lf %lf %lf %lf %lf" % row, file=f)
        rows.append(row)
        x = np.vstack([x, cand.detach().cpu().numpy().reshape(1, -1)])
        fid = np.concatenate([fid, [float(fidelity)]])
        if verbose:
            print("Iter: %d  HV recommendation %.6f  optimal %.6f  feasible %d  points %d/%d  (%.1f s)" %
                  (it, row[0], row[1], row[2], row[4], row[5], time.perf_counter() - t0))
    return rows


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--acq", choices=["jes", "random", "mes"], default="jes")
    ap.add_argument("--epochs", type=int, default=300)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=".")
    ap.add_argument("--num-inducing", type=int, default=None, help="inducing points per surrogate (default: every training row)")
    ap.add_argument("--inducing", choices=["first", "greedy"], default="first",
                    help="with --num-inducing: the first M training rows, or M rows by greedy conditional variance")
    ap.add_argument("--warm-start", action="store_true",
                    help="start every iteration after the first from the previous iteration's fit (warm_start='posterior')")
    ap.add_argument("--warm-epochs", type=int, default=None,
                    help="with --warm-start: phase-2 epochs of a warm refit (default: --epochs)")
    ap.add_argument("--pareto-samples", type=int, default=1,
                    help="average the JES acquisition over this many sampled Pareto sets (one conditioned fit each)")
    ap.add_argument("--pareto-search", choices=["grid", "evolve"], default="grid",
                    help="how the sampled Pareto set is searched: the random grid, or NSGA-II on the GPU started from it")
    ap.add_argument("--recommend-search", choices=["grid", "evolve"], default="grid",
                    help="how the scored recommendation is searched: the random grid, or NSGA-II on the GPU over the "
                         "surrogates' predictions started from it")
    a = ap.parse_args()
    if a.warm_epochs is not None and not a.warm_start:
        ap.error("--warm-epochs needs --warm-start")
    loop_hv(iters=a.iters, acq=a.acq, seed=a.seed, out_dir=a.out, epochs=a.epochs, num_inducing=a.num_inducing,
            inducing=a.inducing, warm_start=a.warm_start, warm_epochs=a.warm_epochs, pareto_samples=a.pareto_samples,
            pareto_search=a.pareto_search, recommend_search=a.recommend_search)
