"""Pareto solution of a sampled multi-objective constrained problem -- host mirror of mobocmf/util/moop.py
(same class surface, same results; the implementation is this build's own).

``MOOP(samples_objs, samples_cons, input_dim, grid_size, pareto_set_size, feasible_values)`` takes posterior function
samples (callables ``f(x: (n, d) ndarray, gradient=False) -> (n,)``, ``gradient=True`` -> (d,) for one point: what
``MFDGP.sample_function_from_each_layer`` returns) and extracts, on a random grid plus the training inputs plus each
objective's constrained optimum, the feasible non-dominated set (objectives are MINIMISED, constraints feasible when
``c(x) >= feasible_value``), optionally thinned to ``pareto_set_size`` points spread over the front.

How it differs inside (results equal the reference's own MOOP, pinned by tests/golden/ref_moop.npz):
  * ``compute_pareto_front``: one stable lexicographic sort, after which every dominator of a row precedes it: a running
    minimum for two objectives, a chunked sweep against the current front otherwise (the reference culls the full array
    once per surviving point);
  * ``compute_pareto_front_and_set_summary_y_space``: farthest-point selection with an incrementally updated
    min-distance vector, O(n) memory (the reference builds the n x n distance matrix);
  * when every sample is a ``layers.rff.RFFChainSample`` on one GPU, the grid is uploaded once and all samples are
    evaluated on it in one launch, the feasibility rule runs there too (``_feasible_grid_batched``); the SLSQP refinements
    stay on the host.  Other samples take the per-callable path;
  * ``refine="device"`` (opt-in; such samples only) replaces the SLSQP run per objective by ONE launch of the multi-start
    augmented-Lagrangian refinement ``functional.rff_refine``: ``refine_starts`` starts per objective, the best feasible grid
    rows, chosen on the device from the grid values that stay there.  The results differ from the default's (other optima
    are found, never worse than the grid's best), so the golden results are pinned with the default only;
  * ``search="evolve"`` (opt-in; such samples only) runs NSGA-II on the GPU from the rows the grid stage found
    (``_evolve_device``, util/pareto_evolve.py) and appends the feasible rows it ends with, so the front weakly dominates
    the default's for the same ``rng``.  It combines with both ``refine`` modes.
"""
import numpy as np
import scipy.optimize as spo
import torch


class NotFeasiblePoints(ValueError):
    pass


def _weakly_dominated_by_any(front, p):
    """True if some row q of ``front`` has q <= p in every objective."""
    return front.shape[0] > 0 and bool(np.any(np.all(front <= p, axis=1)))


class MOOP:

    def __init__(self, samples_objs, samples_cons, input_dim, grid_size=1000, pareto_set_size=None, feasible_values=0.0,
                 min_distance_between_points=1e-6, rng=None, refine="slsqp", refine_starts=16, search="grid",
                 evolve_population=128, evolve_generations=100, evolve_seed=None):
        if refine not in ("slsqp", "device"):
            raise ValueError("refine must be 'slsqp' or 'device' (got %r)" % (refine,))
        if int(refine_starts) < 1:
            raise ValueError("refine_starts must be >= 1")
        if search not in ("grid", "evolve"):
            raise ValueError("search must be 'grid' or 'evolve' (got %r)" % (search,))
        if not 4 <= int(evolve_population) <= 512 or int(evolve_population) % 2:
            raise ValueError("evolve_population must be even, 4..512 (got %r)" % (evolve_population,))
        if int(evolve_generations) < 1:
            raise ValueError("evolve_generations must be >= 1")
        self.search = search
        self.evolve_population, self.evolve_generations = int(evolve_population), int(evolve_generations)
        self.evolve_seed = None if evolve_seed is None else int(evolve_seed)
        self.refine = refine
        self.refine_starts = int(refine_starts)
        self.samples_objs = samples_objs
        self.samples_cons = samples_cons
        self.input_dim = input_dim
        self.bounds = [(0.0, 1.0)] * input_dim
        self.grid_size = grid_size
        self.pareto_set_size = pareto_set_size
        self.min_distance_between_points = min_distance_between_points
        self.feasible_values = feasible_values
        self.rng = rng                    # None: numpy's global generator, as the reference (moop.py:232)

    # ------------------------------------------------------------------ distances
    @staticmethod
    def fast_dist(x1, x2):
        """(len(x2), len(x1)) Euclidean distances, squeezed (reference ``fast_dist`` convention, moop.py:33-39)."""
        diff = x1[None, :, :] - x2[:, None, :]
        return np.sqrt((diff * diff).sum(-1)).squeeze()

    # ------------------------------------------------------------------ feasibility
    def _thresholds(self, n_cons, feasible_values):
        if isinstance(feasible_values, np.ndarray):
            return feasible_values
        return np.full(max(n_cons, self.input_dim), float(feasible_values))

    def find_feasible_grid(self, constraints, grid, feasible_values=0.0, allow_negative_constraints=False):
        """Rows of ``grid`` where every constraint sample is >= its threshold (moop.py:41-72).  With no feasible row:
        None, or -- ``allow_negative_constraints`` -- the rows with the smallest total violation."""
        thr = self._thresholds(len(constraints), feasible_values)
        slack = [c(grid) - thr[i] for i, c in enumerate(constraints)]
        ok = np.ones(grid.shape[0], dtype=bool)
        for s in slack:
            ok &= s >= 0
        if ok.any():
            return grid[ok, :]
        if not allow_negative_constraints:
            return None
        violation = np.zeros(grid.shape[0])
        for s in slack:
            violation += np.minimum(s, 0.0)
        return grid[violation == np.max(violation[violation != 0]), :]

    # ------------------------------------------------------------------ all samples on the grid in one launch
    def _batched_device(self):
        """The GPU every sample lives on when all of them are ``RFFChainSample``s of one GPU, else None (the per-callable
        path)."""
        from ..layers.rff import RFFChainSample
        samples = list(self.samples_objs) + list(self.samples_cons)
        if not samples or not all(isinstance(s, RFFChainSample) for s in samples):
            return None
        devs = {s.device for s in samples}
        dev = devs.pop() if len(devs) == 1 else None
        return dev if dev is not None and dev.type == "cuda" else None

    def _feasible_grid_batched(self, grid, dev, allow_negative_constraints):
        """``find_feasible_grid`` + the objective values on the feasible rows, with the grid uploaded once, every objective
        and constraint sample evaluated in ONE mobocmf_rff_eval_chains launch and the feasibility rule applied on the device
        (mobocmf_rff_feasibility); only the objectives' values and the per-row flags come back.  Returns (grid, evals) or
        (None, None).  What the device refinement needs stays in ``self._grid_dev``: the packed samples, the uploaded grid, the
        objective values and the feasible rows' indices (None on the least-infeasible fallback: no row is a valid start)."""
        from .. import functional as F
        samples = list(self.samples_objs) + list(self.samples_cons)
        n_obj, n_con = len(self.samples_objs), len(self.samples_cons)
        bufs, layers, base = [], [], 0
        for smp in samples:
            b = smp.pack()
            layers.append(smp.layer_offsets(base))
            bufs.append(b)
            base += b.numel()
        params = torch.cat(bufs).to(dev)
        xd = torch.from_numpy(np.ascontiguousarray(grid)).to(dev)
        vals = F.rff_eval_chains(xd, params, layers)
        obj_vals = vals[:n_obj]
        self._grid_dev = {"params": params, "layers": layers, "x": xd, "obj_vals": obj_vals, "rows": None}
        if not n_con:
            self._grid_dev["rows"] = torch.arange(grid.shape[0], device=dev)
            return grid, obj_vals.cpu().numpy().T
        thr = self._thresholds(n_con, self.feasible_values)[:n_con]
        ok, viol = F.rff_feasibility(vals[n_obj:], torch.from_numpy(np.ascontiguousarray(thr, dtype=np.float64)).to(dev))
        ok = ok.cpu().numpy()
        if ok.any():
            rows = np.flatnonzero(ok)
            self._grid_dev["rows"] = torch.from_numpy(rows).to(dev)
        elif not allow_negative_constraints:
            return None, None
        else:
            v = viol.cpu().numpy()
            rows = np.flatnonzero(v == np.max(v[v != 0]))
        return grid[rows, :], obj_vals.cpu().numpy().T[rows]

    # ------------------------------------------------------------------ every objective's constrained optimum in one launch
    def _refine_device(self, evals, feasible_grid):
        """The optima ``optimize_obj_globally`` looks for, all objectives in ONE ``functional.rff_refine`` call: per objective
        the ``refine_starts`` best feasible grid rows (by value, then row index; fewer if fewer rows are feasible) are the
        starts, taken on the device from the grid values kept there.  An optimum is accepted as there: it improves on the
        grid's best value and is feasible (the kernel returns feasible points only).  Returns the list of (1, d) optima."""
        from .. import functional as F
        g = self._grid_dev
        if g["rows"] is None:
            return []
        n_obj, n_con = len(self.samples_objs), len(self.samples_cons)
        rows, R = g["rows"], min(self.refine_starts, int(g["rows"].numel()))
        x0 = []
        for j in range(n_obj):
            order = torch.argsort(g["obj_vals"][j][rows], stable=True)[:R]      # stable: ties in row order
            x0.append(g["x"][rows[order]])
        thr = self._thresholds(n_con, self.feasible_values)[:n_con]
        out = F.rff_refine(torch.stack(x0), g["params"], g["layers"], obj=list(range(n_obj)),
                           cons=[list(range(n_obj, n_obj + n_con))] * n_obj, thr=[thr] * n_obj)
        x_best, f_best = out["x_best"].cpu().numpy(), out["f_best"].cpu().numpy()
        status = out["status"].cpu().numpy()
        return [x_best[j][None] for j in range(n_obj) if status[j] == 0 and f_best[j] < np.min(evals[:, j])]

    # ------------------------------------------------------------------ NSGA-II from the rows found so far
    def _evolve_device(self, grid, evals, seed):
        """``search="evolve"``: the feasible rows assembled so far (grid, training inputs, optima) seed a population that
        ``util.pareto_evolve.ParetoEvolve`` evolves on the GPU for ``evolve_generations`` generations.  Initial population: the
        non-dominated rows, thinned to Np / 2 by ``compute_pareto_front_and_set_summary_y_space`` when there are more, then the
        other rows in row order up to Np = ``evolve_population`` (with fewer rows: the largest even count; fewer than 4, or the
        least-infeasible fallback of the grid: no evolution).  The final rows the device calls feasible and that lie farther
        than 1e-6 from every row are appended with the values the device computed.  Returns (grid, evals)."""
        from .pareto_evolve import ParetoEvolve
        g = self._grid_dev
        if g["rows"] is None or grid.shape[0] < 4:
            return grid, evals
        Np, n = self.evolve_population, grid.shape[0]
        front = np.flatnonzero(self.obtain_indices_pareto(evals))
        if front.size > Np // 2:
            front = self.compute_pareto_front_and_set_summary_y_space(front[:, None], evals[front], Np // 2)[0][:, 0]
        taken = np.zeros(n, dtype=bool)
        taken[front] = True
        rest = np.flatnonzero(~taken)[:max(Np - front.size, 0)]
        rows = np.concatenate((front, rest))
        rows = rows[:rows.size // 2 * 2]
        if rows.size < 4:
            return grid, evals
        n_obj, n_con = len(self.samples_objs), len(self.samples_cons)
        thr = self._thresholds(n_con, self.feasible_values)[:n_con]
        eng = ParetoEvolve(g["params"], g["layers"], n_obj, thr, rows.size, self.input_dim, seed)
        eng.start(torch.from_numpy(np.ascontiguousarray(grid[rows])))
        eng.run(self.evolve_generations)
        out = eng.result()
        X, Fv, viol = out["X"].cpu().numpy(), out["F"].cpu().numpy().T, out["viol"].cpu().numpy()
        new = [i for i in np.flatnonzero(viol == 0.0)
               if not np.isnan(Fv[i]).any() and np.min(np.sqrt(((grid - X[i]) ** 2).sum(1))) > 1e-6]
        if new:
            grid, evals = np.vstack((grid, X[new])), np.vstack((evals, Fv[new]))
        return grid, evals

    # ------------------------------------------------------------------ constrained optimum of one objective
    def _slsqp(self, obj, cons, x0, tol):
        thr = self._thresholds(len(cons), self.feasible_values)
        fun = lambda x: float(np.asarray(obj(x, gradient=False)).reshape(-1)[0])
        jac = lambda x: np.asarray(obj(x, gradient=True)).reshape(-1)
        g = lambda x: np.array([float(np.asarray(c(x, gradient=False)).reshape(-1)[0]) - tol - thr[i]
                                for i, c in enumerate(cons)])
        dg = lambda x: np.stack([np.asarray(c(x, gradient=True)).reshape(-1) for c in cons]) if cons else \
            np.zeros((0, self.input_dim))
        x = spo.fmin_slsqp(fun, x0.copy(), bounds=self.bounds, disp=0, fprime=jac, f_ieqcons=g, fprime_ieqcons=dg)
        x = np.clip(x, 0.0, 1.0)
        return x, fun(x), g(x)

    def optimize_obj_globally(self, obj, cons, obj_evals, feasible_grid, constraint_tol=1e-6):
        """SLSQP from the best grid point; a second, slightly tightened attempt if the first one does not improve on
        the grid or leaves the feasible set (moop.py:74-139).  Returns (1, d) or None."""
        assert self.input_dim == feasible_grid.shape[1]
        best = int(np.argmin(obj_evals))
        x0, f0 = feasible_grid[best, :], float(np.min(obj_evals))
        x, fx, gx = self._slsqp(obj, cons, x0, 0.0)
        if fx < f0 and np.all(gx >= 0):
            return x[None]
        x, fx, gx = self._slsqp(obj, cons, x0, constraint_tol)
        if fx < f0 and np.all(gx >= -constraint_tol):
            return x[None]
        return None

    # ------------------------------------------------------------------ non-dominated set
    @classmethod
    def compute_pareto_front(cls, pts):
        """Boolean mask of the non-dominated rows of ``pts`` (n, k), all objectives minimised.  A row is dropped when
        another row is <= in every objective; of exactly equal rows the first is kept (moop.py:141-166)."""
        pts = np.asarray(pts)
        n = pts.shape[0]
        mask = np.zeros(n, dtype=bool)
        if n == 0:
            return mask
        # lexicographic order, original index as the last key: every (weak) dominator of a row sorts before it
        k = pts.shape[1]
        order = np.lexsort(tuple([np.arange(n)] + [pts[:, j] for j in range(k - 1, -1, -1)]))
        sp = pts[order]
        if k == 1:
            mask[order[0]] = True
            return mask
        if k == 2:        # sorted by f0: a row survives iff its f1 is strictly below everything seen so far
            seen = np.concatenate(([np.inf], np.minimum.accumulate(sp[:-1, 1])))
            mask[order[sp[:, 1] < seen]] = True
            return mask
        front = np.empty((0, k), dtype=pts.dtype)
        for b0 in range(0, n, 256):
            chunk = sp[b0:b0 + 256]
            alive = np.ones(chunk.shape[0], dtype=bool)
            if front.shape[0]:
                alive &= ~(front[None, :, :] <= chunk[:, None, :]).all(2).any(1)
            keep = []
            for i in np.flatnonzero(alive):           # the few survivors against each other, in sorted order
                if not (keep and _weakly_dominated_by_any(chunk[keep], chunk[i])):
                    keep.append(i)
            if keep:
                front = np.concatenate([front, chunk[keep]], 0)
                mask[order[b0 + np.asarray(keep)]] = True
        return mask

    def obtain_indices_pareto(self, pts):
        """Mask in the order ``pts`` was given (moop.py:168-184; the reference pre-sorts for speed only)."""
        return MOOP.compute_pareto_front(pts)

    # ------------------------------------------------------------------ summary of the front
    def compute_pareto_front_and_set_summary_y_space(self, pareto_set, pareto_front, pareto_set_size):
        """At most ``pareto_set_size`` points: the best of every objective first, then repeatedly the point of the front
        farthest (in objective space) from those already chosen (moop.py:186-219)."""
        assert pareto_set_size > 0
        n, k = pareto_front.shape
        if n <= pareto_set_size:
            return pareto_set, pareto_front
        chosen = np.zeros(pareto_set_size, dtype=np.int64)
        min_dist = np.full(n, np.inf)

        def add(pos, idx):
            chosen[pos] = idx
            diff = pareto_front - pareto_front[idx]
            np.minimum(min_dist, np.sqrt((diff * diff).sum(1)), out=min_dist)

        for j in range(k):
            add(j, int(np.argmin(pareto_front[:, j])))
        for pos in range(k, pareto_set_size):
            add(pos, int(np.argmax(min_dist)))
        return pareto_set[chosen, :], pareto_front[chosen, :]

    # ------------------------------------------------------------------ the whole extraction
    def compute_pareto_solution_from_samples(self, inputs, allow_negative_constraints=False):
        """(pareto_set, pareto_front, samples_objs, samples_cons) as torch float64 / the callables, or None when the
        sampled constraints leave no feasible grid point (moop.py:221-286)."""
        inputs = np.asarray(inputs, dtype=np.float64)
        n_rand = self.input_dim * self.grid_size
        rand = np.random.uniform(size=(n_rand, self.input_dim)) if self.rng is None else \
            self.rng.uniform(size=(n_rand, self.input_dim))
        grid = np.concatenate((rand, inputs))
        dev = self._batched_device()
        if self.search == "evolve":
            if dev is None:
                raise ValueError("MOOP(search='evolve') needs every sample to be an RFFChainSample on one GPU "
                                 "(layers.rff.sample_chain_from_posterior); there is no host fallback")
            seed = self.evolve_seed               # drawn after the grid, and in this mode only: the default's draws stay
            if seed is None:
                seed = int(np.random.randint(0, 2 ** 63 - 1, dtype=np.int64)) if self.rng is None else \
                    int(self.rng.integers(0, 2 ** 63 - 1))
        if self.refine == "device" and dev is None:
            raise ValueError("MOOP(refine='device') needs every sample to be an RFFChainSample on one GPU "
                             "(layers.rff.sample_chain_from_posterior); there is no host fallback")
        if dev is not None:
            grid, evals = self._feasible_grid_batched(grid, dev, allow_negative_constraints)
            if grid is None:
                return None
        else:
            grid = self.find_feasible_grid(self.samples_cons, grid, feasible_values=self.feasible_values,
                                           allow_negative_constraints=allow_negative_constraints) \
                if len(self.samples_cons) else grid
            if grid is None:
                return None
            evals = np.stack([np.asarray(obj(grid)).reshape(-1) for obj in self.samples_objs], 1)
        if self.refine == "device":
            optima = self._refine_device(evals, grid)
        else:
            optima = [self.optimize_obj_globally(obj, self.samples_cons, evals[:, j], grid)
                      for j, obj in enumerate(self.samples_objs)]
        extra = []
        for opt in optima:
            if opt is not None and np.min(np.sqrt(((grid - opt) ** 2).sum(1))) > 1e-6:
                extra.append(opt)
        if extra:
            extra = np.concatenate(extra, 0)
            grid = np.vstack((grid, extra))
            evals = np.vstack((evals, np.stack([np.asarray(obj(extra)).reshape(-1) for obj in self.samples_objs], 1)))
        if self.search == "evolve":
            grid, evals = self._evolve_device(grid, evals, seed)
        keep = self.obtain_indices_pareto(evals)
        pareto_set, pareto_front = grid[keep, :], evals[keep, :]
        if self.pareto_set_size is not None:
            pareto_set, pareto_front = self.compute_pareto_front_and_set_summary_y_space(pareto_set, pareto_front,
                                                                                        self.pareto_set_size)
        return torch.from_numpy(pareto_set), torch.from_numpy(pareto_front), self.samples_objs, self.samples_cons
