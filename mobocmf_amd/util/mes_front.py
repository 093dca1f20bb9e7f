"""The best objective values of a max-value entropy search iteration on the exact-GP baselines: one sampled Pareto front of the
posterior function samples of all black-boxes (util/exact_sample.py draws them, util/moop.py extracts the front).

Convention.  MES maximises: ``MESMOC_MFGP`` scores a point by the entropy of an objective truncated BELOW its best value, so the
objective models are fitted to the NEGATED observations of a minimised black-box, and ``best_objective_values`` are maxima of
those models' samples.  A constraint is feasible when its value is at least its threshold (``constraint_thresholds``), as in
``MESMOC_MFGP``'s probability of feasibility.  ``MOOP`` minimises, so it is handed the negated objective samples and the
constraint samples with the thresholds as ``feasible_values``; with ``pareto_front`` its front,

    best_objective_values[name] = -min(pareto_front[:, column of name]).
"""
import numpy as np

from .exact_sample import draw_chain_samples
from .moop import MOOP, NotFeasiblePoints

MAX_TRIES_FOR_FEASIBLE_GRID = 50      # (MFDGPHandler.MAX_TRIES_FOR_FEASIBLE_GRID)


class SampledFront:
    """``best_objective_values`` {objective: float}; ``pareto_set`` / ``pareto_front`` (torch float64; the front in MOOP's
    minimised convention, a column per objective in the order given); ``samples_objs`` / ``samples_cons`` {name: the
    ``RFFChainSample`` drawn, objectives NOT negated}; ``tries`` the constraint draws made; ``fallback`` whether the least
    infeasible rows had to serve; ``engines`` {name: "host" / "device"}."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def sample_pareto_front(objectives, constraints, constraint_thresholds, inputs, num_fidelities, nFeatures=500, generator=None,
                        rng=None, engine="device", max_tries=MAX_TRIES_FOR_FEASIBLE_GRID, **moop_kwargs):
    """Draws one top-fidelity function sample per model (``objectives`` / ``constraints``: {name: ``MFGP`` or ``MFGP_lin``},
    the objective models fitted to the negated observations -- see the module's convention) and extracts the sampled problem's
    Pareto front on a random grid plus ``inputs`` (the training inputs, (n, d) in [0, 1]^d).  When no grid row is feasible the
    constraint samples are drawn afresh, up to ``max_tries`` times; after that the least infeasible rows of the last samples
    serve (``allow_negative_constraints``) -- the policy of ``BlackBoxMFDGPFitter._sample_and_store_pareto_solution``.
    ``rng``: the numpy generator of MOOP's grid; ``moop_kwargs`` (``grid_size``, ``pareto_set_size``, ``refine``, ``search``,
    ``evolve_*`` ...) pass through, so with ``refine="device"`` / ``search="evolve"`` the whole stage stays on the GPU.
    Returns a ``SampledFront``."""
    if engine not in ("host", "device"):
        raise ValueError("sample_pareto_front: engine is \"host\" or \"device\" (got %r)" % (engine,))
    if not objectives:
        raise ValueError("sample_pareto_front: at least one objective")
    top = int(num_fidelities) - 1
    inputs = np.asarray(inputs, dtype=np.float64)
    obj_names, con_names = list(objectives), list(constraints)
    thr = np.array([float(constraint_thresholds[k]) for k in con_names], dtype=np.float64)
    drawn = draw_chain_samples(objectives, top, nFeatures=nFeatures, generator=generator, engine=engine)
    engines = dict(drawn.engines)
    samples_objs = {k: drawn.samples[k] for k in obj_names}
    negated = [samples_objs[k].negated() for k in obj_names]
    tries, res, optimizer, samples_cons, fallback = 0, None, None, {}, False
    for _ in range(max(1, int(max_tries)) if con_names else 1):
        tries += 1
        if con_names:
            drawn = draw_chain_samples(constraints, top, nFeatures=nFeatures, generator=generator, engine=engine)
            engines.update(drawn.engines)
            samples_cons = {k: drawn.samples[k] for k in con_names}
        optimizer = MOOP(negated, [samples_cons[k] for k in con_names], input_dim=inputs.shape[1], feasible_values=thr, rng=rng,
                         **moop_kwargs)
        res = optimizer.compute_pareto_solution_from_samples(inputs)
        if res is not None:
            break
    else:
        fallback = True
        res = optimizer.compute_pareto_solution_from_samples(inputs, allow_negative_constraints=True)
        if res is None:
            raise NotFeasiblePoints("[ERROR] No feasible points were found in the constraint space! # tries: %d." % tries)
    pareto_set, pareto_front = res[0], res[1]
    best = {k: -float(pareto_front[:, j].min()) for j, k in enumerate(obj_names)}
    return SampledFront(best_objective_values=best, pareto_set=pareto_set, pareto_front=pareto_front, samples_objs=samples_objs,
                        samples_cons=samples_cons, tries=tries, fallback=fallback, engines=engines)
