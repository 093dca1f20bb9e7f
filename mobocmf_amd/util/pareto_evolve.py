"""NSGA-II over chain samples with no host in the loop: ``MOOP(search="evolve")`` and ``functional.rff_evolve``.

The population logic is csrc/pareto_evolve.hip (include/mobocmf_hip.h states it); the objective and constraint values come
from the launches MOOP's grid stage already uses.  One generation is, in stream order,

    mobocmf_nsga_vary (Np children of the ranked parents, rows Np .. 2 Np - 1 of the row buffer)
    -> mobocmf_rff_eval_chains on the children only  -> mobocmf_rff_feasibility
    -> two element-wise copies (the children's objective values beside the parents', the violation with its sign turned)
    -> mobocmf_nsga_survive on the 2 Np rows, in place: the survivors are rows 0 .. Np - 1 again, and the launch increments
       the generation word that the next vary draws with

captured once per engine as a HIP graph -- a single chain of nodes, no parallel branches -- and replayed; the host reads
nothing until the caller fetches the result.  Limits: Np even in 4..512 (the survive launch ranks 2 Np <= 1024 rows on one
workgroup), one GPU, one process, chain samples only.

``NsgaEngine`` is everything but the evaluation: util/recommend_evolve.py evolves against fitted surrogates on it.
"""
import ctypes

import numpy as np
import torch

from .. import _lib
from .. import functional as F

MIN_POPULATION, MAX_POPULATION = 4, _lib.NSGA_MAX_ROWS // 2


class NsgaEngine:
    """The buffers and the captured generation of one search over a population ``Np`` x ``d`` with ``n_obj`` objectives
    (minimised) and ``n_con`` constraints: the 2 Np row buffers, the survive and vary launches, the graph.  A subclass supplies
    ``_evaluate(row0)``: the objective values and violations (>= 0, 0 = feasible) of rows [row0, row0 + Np) of ``X`` into
    ``F[:, row0:row0 + Np]`` and ``viol[row0:row0 + Np]``, in launches on the current stream that read nothing on the host.
    ``seed`` is the Philox key of every draw, ``options`` the ``functional.nsga_options``.

    ``start(x0)`` evaluates and ranks the initial population (one rank-only survive); ``run(g)`` advances g generations: the
    first one of an engine is issued eagerly, the others are replays; ``result()`` returns device tensors.  ``use_graph =
    False`` issues every generation eagerly (tests, A/B)."""
    use_graph = True

    def _allocate(self, Np, d, n_obj, n_con, seed, options, dev):
        """The checks on Np and d and the buffers; returns the zero-filled allocator on ``dev``."""
        who = type(self).__name__
        if not MIN_POPULATION <= Np <= MAX_POPULATION or Np % 2:
            raise ValueError("%s: the population is even, %d..%d (got %d)" % (who, MIN_POPULATION, MAX_POPULATION, Np))
        if not 1 <= d <= _lib.MAX_D:
            raise ValueError("%s: d in 1..%d" % (who, _lib.MAX_D))
        self.lib = _lib.require_device()
        self.Np, self.d, self.n_obj, self.n_con = Np, d, n_obj, n_con
        self.seed = int(seed) & (2 ** 64 - 1)
        self.options = F._nsga_opt(options)
        z = lambda *shape, dtype=torch.float64: torch.zeros(*shape, dtype=dtype, device=dev)
        self.X, self.F = z(2 * Np, d), z(n_obj, 2 * Np)
        self.viol = z(2 * Np) if n_con else None
        self.rank, self.crowd, self.src = z(Np, dtype=torch.int32), z(Np), z(Np, dtype=torch.int32)
        self.generation = z(1, dtype=torch.int64)
        self._graph = None
        self._stream = None      # the capture's stream
        self._started = self._warm = False
        return z

    # ------------------------------------------------------------------ the launches
    def _evaluate(self, row0):
        """Objective values and violations of rows [row0, row0 + Np) into the row buffers."""
        raise NotImplementedError

    def _survive(self, n_in, generation):
        p = F._ptr
        _lib.check(self.lib.mobocmf_nsga_survive(n_in, self.Np, self.d, self.n_obj, p(self.X), p(self.F), 2 * self.Np,
                                                 p(self.viol), p(self.X), p(self.F), 2 * self.Np, p(self.viol), p(self.rank),
                                                 p(self.crowd), p(self.src), p(generation), F._stream()),
                   "mobocmf_nsga_survive")

    def _vary(self):
        p, Np = F._ptr, self.Np
        _lib.check(self.lib.mobocmf_nsga_vary(Np, self.d, p(self.X), p(self.rank), p(self.crowd), self.seed,
                                              p(self.generation), None if self.options is None else ctypes.byref(self.options),
                                              p(self.X[Np:]), None, F._stream()), "mobocmf_nsga_vary")

    def _generation(self):
        self._vary()
        self._evaluate(self.Np)
        self._survive(2 * self.Np, self.generation)

    # ------------------------------------------------------------------ the search
    def start(self, x0):
        """``x0`` (Np, d): the initial population; it is evaluated and ranked, the generation word returns to 0."""
        with torch.no_grad(), torch.cuda.device(self.X.device):
            x0 = torch.as_tensor(x0, dtype=torch.float64).reshape(self.Np, self.d)
            self.X[:self.Np].copy_(x0)
            self.generation.zero_()
            self._evaluate(0)
            self._survive(self.Np, None)
            self._started = True

    def run(self, generations):
        generations = int(generations)
        if generations < 0 or not self._started:
            raise ValueError("%s.run: start(x0) first, generations >= 0" % type(self).__name__)
        with torch.no_grad(), torch.cuda.device(self.X.device):
            left = generations
            if left and not self._warm:       # eagerly once: the kernels are loaded and configured outside a capture
                self._generation()
                self._warm = True
                left -= 1
            if not self.use_graph:
                for _ in range(left):
                    self._generation()
                return
            if left and self._graph is None:
                self._stream = torch.cuda.Stream(device=self.X.device)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=self._stream, capture_error_mode="thread_local"):
                    self._generation()
                self._graph = g
            for _ in range(left):
                self._graph.replay()

    def result(self):
        """The population as it stands (clones): X (Np, d), F (n_obj, Np), viol (Np,), rank, crowd, generation."""
        Np = self.Np
        viol = self.viol[:Np].clone() if self.n_con else torch.zeros(Np, dtype=torch.float64, device=self.X.device)
        return {"X": self.X[:Np].clone(), "F": self.F[:, :Np].clone(), "viol": viol, "rank": self.rank.clone(),
                "crowd": self.crowd.clone(), "generation": self.generation.clone()}


class ParetoEvolve(NsgaEngine):
    """``NsgaEngine`` over chain samples ``params`` / ``layers`` (as ``functional.rff_eval_chains``), the first ``n_obj`` of them
    objectives (minimised), the rest constraints, feasible when sample >= ``thr``."""

    def __init__(self, params, layers, n_obj, thr, Np, d, seed, options=None):
        self.lib = _lib.require_device()
        Np, d, n_obj = int(Np), int(d), int(n_obj)
        K = len(layers)
        if not 1 <= n_obj <= min(K, _lib.PARETO_MAX_K):
            raise ValueError("ParetoEvolve: 1..%d objectives among the %d samples (got %d)" % (_lib.PARETO_MAX_K, K, n_obj))
        if not torch.is_tensor(params) or params.dim() != 1 or params.device.type != "cuda" or params.dtype != torch.float64:
            raise _lib.MobocmfError("ParetoEvolve: params must be a 1-D float64 tensor on a GPU")
        dev = params.device
        z = self._allocate(Np, d, n_obj, K - n_obj, seed, options, dev)
        self.K = K
        self.params = params.detach().contiguous()
        self.desc = F._rff_chain_table("ParetoEvolve", layers, d, self.params.numel(), dev)
        self.vals = z(K, Np)
        if self.n_con:
            thr = torch.as_tensor(np.asarray(thr, dtype=np.float64).reshape(-1)).to(dev)
            if thr.numel() != self.n_con:
                raise ValueError("ParetoEvolve: one threshold per constraint sample")
            self.thr, self.ok, self.viol_raw = thr.contiguous(), z(Np, dtype=torch.int32), z(Np)

    def _evaluate(self, row0):
        Np, lib, p, st = self.Np, self.lib, F._ptr, F._stream()
        x = self.X[row0:row0 + Np]
        _lib.check(lib.mobocmf_rff_eval_chains(self.K, self.d, Np, p(x), p(self.params), self.params.numel(), p(self.desc),
                                               p(self.vals), st), "mobocmf_rff_eval_chains")
        if self.n_con:
            _lib.check(lib.mobocmf_rff_feasibility(self.n_con, Np, p(self.vals[self.n_obj:]), Np, p(self.thr), p(self.ok),
                                                   p(self.viol_raw), st), "mobocmf_rff_feasibility")
            torch.neg(self.viol_raw, out=self.viol[row0:row0 + Np])
        self.F[:, row0:row0 + Np].copy_(self.vals[:self.n_obj])
