"""Max-value entropy search on the exact-GP baselines -- host mirror of mobocmf/acquisition_functions/MESMOC_MFGP.py
(``_MES_MFGP.forward`` :38-71, ``MESMOC_MFGP`` :75-157).  SURVEY row N4: a comparison baseline, plain float64 torch;
botorch's ``optimize_acqf`` is replaced by the same batched multi-start projected Adam as in JESMOC_MFDGP.

``MESMOC_MFGP(search="device")`` keeps that search on the GPU: the models' moments and input gradients from mobocmf_exact_predict
against factorisations formed once, the MES value and its seeds from mobocmf_mes_group_forward."""
import math

import torch

from .JESMOC_MFDGP import optimize_acqf_multistart

CLAMP_LB = torch.finfo(torch.float32).eps


def _ncdf(z):
    return 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0)))


class _MES_MFGP:

    def __init__(self, fidelity, model, best_value, is_constraint):
        self.fidelity, self.model, self.best_value, self.is_constraint = fidelity, model, best_value, is_constraint

    def forward(self, X):
        """:38-71 -- moments of the truncated Gaussian below the best value, then the noise; constraints: P(feasible)."""
        pred = self.model.predict(X, self.fidelity)
        mean, var = pred.mean, pred.variance
        stdv = var.sqrt()
        z = (self.best_value - mean) / stdv
        if self.is_constraint:
            return 1.0 - _ncdf(z)
        cdf = _ncdf(z).clamp_max(1 - CLAMP_LB)
        pdf = torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
        ratio = pdf / (1.0 - cdf)
        noise = self.model.likelihood.noise.reshape(())
        var_trunc = var * (1 + (z - ratio) * ratio).clamp_min(CLAMP_LB) + noise
        return torch.clamp(0.5 * torch.log(var + noise) - 0.5 * torch.log(var_trunc), min=0.0)

    __call__ = forward


class MESMOC_MFGP:
    """``search="device"``: a fidelity whose models -- the objectives at that level, then the constraints of the TOP level, the
    models ``coupled_acq`` evaluates -- all fit ``ExactGPPredictGroup`` (util/exact_predict.py: on the GPU, n <= 512) is searched
    by ``MesDeviceAcqSearch`` (util/acq_search.py), one graph replay per iterate against factorisations formed once; any other
    fidelity runs the host loop.  ``last_search_engine[fidelity]`` says which; with ``"device"``, ``last_search_values[fidelity]``
    and ``last_search_candidates[fidelity]`` are every fidelity's winner, read from the device once per call."""

    search = "host"           # (class defaults: what an object made with __new__ has)
    num_restarts, raw_samples, search_lr = 5, 200, 0.02

    def __init__(self, objectives, constraints, input_dim, num_fidelities, best_objective_values, constraint_thresholds,
                 standard_bounds=None, search="host"):
        self.search = search
        self.last_search_engine = {}      # fidelity -> "host" / "device": the engine its last search ran on
        self.standard_bounds = standard_bounds
        self.num_fidelities, self.input_dim = num_fidelities, input_dim
        self.objectives, self.constraints = objectives, constraints
        self.best_objective_values, self.constraint_thresholds = best_objective_values, constraint_thresholds
        self.costs_blackboxes, self.acquisition_objs, self.acquisition_cons = {}, {}, {}
        for n_f in range(num_fidelities):
            self.acquisition_objs[n_f], self.acquisition_cons[n_f] = {}, {}
            self.costs_blackboxes[n_f] = {"total": 0.0}

    def add_blackbox(self, fidelity, blackbox_name, cost_evaluation=1.0, is_constraint=False):
        if not is_constraint:
            acq = _MES_MFGP(fidelity, self.objectives[blackbox_name], self.best_objective_values[blackbox_name], False)
            self.acquisition_objs[fidelity][blackbox_name] = acq
            self.costs_blackboxes[fidelity]["total"] += cost_evaluation
            self.costs_blackboxes[fidelity][blackbox_name] = cost_evaluation
        else:
            acq = _MES_MFGP(fidelity, self.constraints[blackbox_name], self.constraint_thresholds[blackbox_name], True)
            self.acquisition_cons[fidelity][blackbox_name] = acq
        return acq

    def coupled_acq(self, X, fidelity):
        """:120-132: sum of the objectives' MES at ``fidelity`` times the probability of feasibility at the HIGHEST one."""
        X = X.double()
        acq = torch.zeros(X.shape[0], dtype=X.dtype, device=X.device)
        for a in self.acquisition_objs[fidelity].values():
            acq = acq + a(X)
        feas = torch.ones(X.shape[0], dtype=X.dtype, device=X.device)
        for a in self.acquisition_cons[self.num_fidelities - 1].values():
            feas = feas * a(X)
        return acq * feas

    def _group_models(self, fidelity):
        """(models, levels, best values, n_obj, n_con) of the models ``coupled_acq`` evaluates at ``fidelity``: the objectives at
        that level, then the constraints of the top level."""
        objs = list(self.acquisition_objs[fidelity].values())
        cons = list(self.acquisition_cons[self.num_fidelities - 1].values())
        return ([a.model for a in objs + cons], [fidelity] * len(objs) + [self.num_fidelities - 1] * len(cons),
                [a.best_value for a in objs + cons], len(objs), len(cons))

    def _device_search(self, fidelity):
        """(MesDeviceAcqSearch, raw-candidate group) of ``fidelity`` when all its models fit ExactGPPredictGroup, else None:
        the host engine.  Engine and groups are built once per fidelity and set of models."""
        from .. import _lib
        from ..util.acq_search import MesDeviceAcqSearch
        from ..util.exact_predict import ExactGPPredictGroup
        bounds = self.standard_bounds
        models, levels, best, n_obj, n_con = self._group_models(fidelity)
        R, n_raw = self.num_restarts, self.raw_samples
        if bounds is None or not bounds.is_cuda or bounds.dtype != torch.float64 or n_obj < 1:
            return None
        if len(models) > 2 * _lib.ACQ_MAX_PAIRS or not R <= n_raw <= _lib.TOPK_MAX_N or R > _lib.TOPK_MAX_K:
            return None
        d = bounds.shape[1]
        if any(ExactGPPredictGroup.why_not(m, l, T, d) is not None for m, l in zip(models, levels) for T in (R, n_raw)):
            return None
        cache = self.__dict__.setdefault("_device_searches", {})
        # (the training rows are part of the key: a captured iterate carries the launch geometry of the n it was captured with)
        key = (tuple((id(m), m.x_train.shape[0]) for m in models), tuple(levels), R, n_raw, d, bounds.data_ptr())
        best = torch.stack([torch.as_tensor(b, dtype=torch.float64).detach().reshape(()).to(bounds.device) for b in best])
        if fidelity not in cache or cache[fidelity][0] != key:
            grp = ExactGPPredictGroup(models, levels, R, d)
            raw = ExactGPPredictGroup(models, levels, n_raw, d, want_gradients=False)
            cache[fidelity] = (key, MesDeviceAcqSearch(grp, bounds, R, self.search_lr, best, n_obj, n_con), raw)
        _, engine, raw = cache[fidelity]
        engine.best.copy_(best)      # (the best values may have moved since the engine was built)
        return engine, raw

    def _search_on_device(self, maxiter, generator):
        """Every fidelity's search with the winners left on the device, then ONE read of them and of the factorisations'
        verdicts; the weighting and the choice are the loop of ``get_nextpoint_coupled`` on host doubles.  A fidelity that
        does not fit the device engine runs the host loop and says so in ``last_search_engine``."""
        from ..util.acq_search import raise_on_info
        from .JESMOC_MFDGP import _read_once
        engines = self.__dict__.setdefault("last_search_engine", {})
        found, used = [], []
        try:
            for fidelity in range(self.num_fidelities):
                route = self._device_search(fidelity)
                if route is None:
                    engines[fidelity] = "host"
                    found.append(self._search_on_host(fidelity, maxiter, generator))
                    continue
                engine, raw = route
                used.append(engine)
                lo, hi = self.standard_bounds[0], self.standard_bounds[1]
                with torch.no_grad():      # the draw of optimize_acqf_multistart: both engines see the same points
                    Xraw = lo + (hi - lo) * torch.rand(self.raw_samples, lo.numel(), dtype=lo.dtype, device=lo.device,
                                                       generator=generator)
                    engine.start_from_raw(raw, Xraw)
                    engines[fidelity] = "device"
                    found.append(engine.run(None, maxiter))
            vals = torch.stack([v.detach().reshape(()).double() for _, v in found])
            host, words = _read_once(vals, torch.cat([e.info_words() for e in used]) if used else None)
            if words is not None:
                raise_on_info(words, "device acquisition search")
        finally:
            for engine in used:      # (after the read: the launches are done with the factorisations)
                for grp in (engine.group, engine.__dict__.get("raw_group")):
                    if grp is not None:
                        grp.thaw()
        self.last_search_values = {f: float(host[f]) for f in range(self.num_fidelities)}
        self.last_search_candidates = {f: found[f][0] for f in range(self.num_fidelities)}
        best = None
        for fidelity, (cand, _) in enumerate(found):
            w = float(host[fidelity]) / self.costs_blackboxes[fidelity]["total"]
            if best is None or best[0] < w:
                best = (w, cand, fidelity)
        return best

    def _search_on_host(self, fidelity, maxiter, generator):
        return optimize_acqf_multistart(lambda x: self.coupled_acq(x, fidelity=fidelity), self.standard_bounds,
                                        num_restarts=self.num_restarts, raw_samples=self.raw_samples, maxiter=maxiter,
                                        lr=self.search_lr, generator=generator)

    def get_nextpoint_coupled(self, iteration=None, verbose=False, maxiter=200, generator=None):
        """:134-157: best cost-weighted candidate over the fidelities.  ``generator``: the raw candidates' draw (either engine)."""
        if self.search not in ("host", "device"):
            raise ValueError("search must be 'host' or 'device' (got %r)" % (self.search,))
        if self.search == "device":
            best = self._search_on_device(maxiter, generator)
        else:
            best = None
            engines = self.__dict__.setdefault("last_search_engine", {})
            for fidelity in range(self.num_fidelities):
                engines[fidelity] = "host"
                cand, val = self._search_on_host(fidelity, maxiter, generator)
                w = val / self.costs_blackboxes[fidelity]["total"]
                if best is None or best[0] < w:
                    best = (w, cand, fidelity)
        w, cand, fidelity = best
        if verbose:
            print("Iter:", iteration, "Acquisition:", float(w * self.costs_blackboxes[fidelity]["total"]),
                  " Evaluating fidelity", fidelity, "at", cand[0].cpu().numpy())
        return cand[0, :], fidelity
