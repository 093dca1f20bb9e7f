"""The acquisition search with no host in the loop: ``JESMOC_MFDGP(search="device")``.

``optimize_acqf_multistart`` (acquisition_functions/JESMOC_MFDGP.py) drives its ~200 iterates per fidelity from Python: around
the two one-launch model evaluations of a predict group (util/tiny_step.py TinyPredictGroup, util/coop_step.py CoopPredictGroup)
it issues a dozen element-wise framework kernels, three copies and an optimiser launch pair, and an evaluation costs more host
time than device time.  ``DeviceAcqSearch`` keeps the same search on the GPU (csrc/acq_search.hip): one iterate is FOUR launches
in stream order --

    group STEP_FORWARD  ->  mobocmf_jes_mc_group_forward (value, seeds, best iterate; K sampled Pareto sets, K = 1 being
    mobocmf_jes_group_forward)  ->  group STEP_INPUT_GRADIENTS  ->  mobocmf_ascent_adam_step (the iterate IS the group's x buffer)

-- captured once as a HIP graph (a single chain, no parallel branches) and replayed; nothing is read on the host until the
caller fetches the winner.

``DecoupledDeviceAcqSearch`` runs the searches of all black-boxes of a fidelity at once, each for its own JES term
(``JESMOC_MFDGP.get_nextpoint_decoupled``): the same chain with mobocmf_jes_mc_box_forward in the JES position.

``MesDeviceAcqSearch`` is the coupled search of the MES baseline over exact-GP surrogates (``MESMOC_MFGP(search="device")``): the
same chain over an ExactGPPredictGroup (util/exact_predict.py) with mobocmf_mes_group_forward in the JES position.
"""
import torch

from .. import _lib
from .. import functional as F


class DeviceAcqSearch:
    """Projected-Adam multi-start ascent of the coupled JES acquisition over ``group`` -- a PredictGroup (util/predict_group.py)
    for T = ``num_restarts`` test points (JESMOC_MFDGP._tiny_group / _panel_group) -- inside the box ``bounds`` (2, d).  ``lr`` is
    scaled by mean(hi - lo) as the host loop does.  ``num_pareto_samples`` = K: black-box p owns the models p (1 + K)
    (unconditioned) and p (1 + K) + 1 + k (conditioned on sampled Pareto set k); the JES launch, mobocmf_jes_mc_group_forward,
    averages over the K (K = 1: models 2p / 2p + 1, the reference's estimator).

    ``run(x0, maxiter)`` -> device tensors (candidate (1, d), value ()), WITHOUT synchronising: X_0 ... X_maxiter are each
    scored once, the best iterate of every restart is kept, the best of those is returned.  The first iterate of a search runs
    eagerly (a frozen CoopPredictGroup forms its chains there, so the replayed launches carry STEP_CHAIN_VALID); the others are
    replays of the captured iterate(s).  The group is frozen by ``run``, and the raw-candidate group by ``start_from_raw``
    (``self.raw_group``); neither is thawed here, because a cooperative group's ``thaw()`` reads the status word and that read
    synchronises.  The caller thaws BOTH once it has fetched the result (``group.thaw()`` reports an abandoned in-launch
    wait; JESMOC_MFDGP does it for every group it built): a group left frozen keeps chains of parameters that may since have
    changed.  ``info_words()`` are the models' Cholesky verdicts."""
    use_graph = True          # False: the same launches issued eagerly (tests, A/B)
    iters_per_graph = 1       # iterates unrolled into one graph (DESIGN.md 5.6 on what tools/acq_search_bench.py reports)

    def __init__(self, group, bounds, num_restarts, lr, betas=(0.9, 0.999), eps=1e-8, num_pareto_samples=1, n_searches=None):
        """``n_searches`` = B: the engine runs B independent searches of R = ``num_restarts`` rows each, rows [p R, (p + 1) R) of
        the group's x being search p's (the raw candidates are shared, the restarts and the winner are chosen per search).  None:
        the coupled search, B = 1, whose results come without the leading axis of the searches."""
        _lib.require_device()
        K = self.K = int(num_pareto_samples)
        if K < 1:
            raise ValueError("DeviceAcqSearch: num_pareto_samples >= 1 (got %d)" % K)
        B, R = self.B, self.R = int(n_searches or 1), int(num_restarts)
        self._one = (lambda t: t[0]) if n_searches is None else (lambda t: t)
        self._check_group(group)
        dev, T, d = group.device, group.T, group.d
        self.group, self.T, self.d = group, T, d
        self.lo = bounds[0].detach().to(dev, torch.float64).contiguous()
        self.hi = bounds[1].detach().to(dev, torch.float64).contiguous()
        self.lr = float(lr) * float((bounds[1] - bounds[0]).mean())      # (construction only: the one host read of the bounds)
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        z = lambda *shape: torch.zeros(*shape, dtype=torch.float64, device=dev)
        self.noise = group.noise().detach().clone().contiguous()
        self.acq, self.best_v, self.best_x = z(T), z(T), z(T, d)
        self.exp_avg, self.exp_avg_sq = z(T, d), z(T, d)
        self.steps_done = torch.zeros(1, dtype=torch.int64, device=dev)
        self.win_v, self.win_i, self.cand = z(B), torch.zeros(B, dtype=torch.int64, device=dev), z(B, d)
        self._graphs, self._raw = {}, {}
        self._capture_stream = group.stream

    def _check_group(self, group):
        """What the acquisition launch (``_jes``) asks of the group's models; a subclass with another launch has another rule."""
        K = self.K
        if group.T != self.B * self.R or len(group.models) % (1 + K):
            raise _lib.MobocmfError("DeviceAcqSearch: a group of (uncond, cond_1 .. cond_K) per black-box built for T = "
                                    "num_restarts test points")
        if not 1 + K <= len(group.models) <= 2 * _lib.ACQ_MAX_PAIRS:
            raise _lib.MobocmfError("DeviceAcqSearch: 1 + K..%d models per group" % (2 * _lib.ACQ_MAX_PAIRS))

    # ------------------------------------------------------------------ the launches
    def _jes(self, grp, noise, acq, **track):
        """The acquisition launch of an iterate -- here the JES launch on ``grp``'s moments; a subclass puts its own in this
        position (MesDeviceAcqSearch).  ``track`` (seeds, x, best_v, best_x): an iterate, ``acq`` (T,); none: a chunk of
        raw candidates, ``acq`` (B, chunk) -- here B = 1, the coupled value."""
        F.jes_mc_group_forward(grp.moments, noise, self.K, grp.T, grp.S, acq, stream=grp.stream, **track)

    def _score(self, seeds):
        """The forward launch and the JES kernel on the group's current x: acq, the best iterate so far, optionally the seeds."""
        g = self.group
        g._launch(_lib.STEP_FORWARD)
        self._jes(g, self.noise, self.acq, seeds=g.seeds if seeds else None, x=g.x, best_v=self.best_v, best_x=self.best_x)

    def _iterate(self):
        """One iterate: four launches (on the group's stream; None: the current one)."""
        g = self.group
        self._score(seeds=True)
        g._launch(_lib.STEP_INPUT_GRADIENTS)
        F.ascent_adam_step(g.x, g.gx, self.lo, self.hi, self.exp_avg, self.exp_avg_sq, self.steps_done, self.lr, self.betas,
                           self.eps, stream=g.stream)

    def _graph(self, n):
        """``n`` iterates captured once (as TinyConditionedStep._capture): every argument is static and the step count lives on
        the device, so a replay IS the next n iterates.  The capture pass itself executes nothing."""
        if n not in self._graphs:
            if self._capture_stream is None:
                self._capture_stream = torch.cuda.Stream(device=self.group.device)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=self._capture_stream, capture_error_mode="thread_local"):
                for _ in range(n):
                    self._iterate()
            self._graphs[n] = g
        return self._graphs[n]

    def _stream_ctx(self):
        s = self.group.stream
        return torch.cuda.stream(s if s is not None else torch.cuda.current_stream(self.group.device))

    # ------------------------------------------------------------------ the search
    def start_from_raw(self, raw_group, Xraw):
        """Scores the raw candidates ``Xraw`` (n, d) through ``raw_group`` -- the same models for T = n test points, or for
        T = n / c: c equal chunks, one forward launch each, where n S columns are beyond the one-launch kernels' limit --
        ONCE for all B searches (one JES launch per chunk: row p of ``vals`` (B, n) is search p's value at every candidate) and
        writes each search's R best rows straight into rows [p R, (p + 1) R) of the search group's x, one selection per search.
        Returns (vals (B, n), the restarts' values (B, R), their indices (B, R)) -- coupled: (n,), (R,), (R,) -- device tensors
        of this object, overwritten by the next call.  A cooperative ``raw_group`` is left frozen (see the class docstring): the
        caller thaws it with the search group."""
        n, Tc, B, R = Xraw.shape[0], raw_group.T, self.B, self.R
        if n % Tc or len(raw_group.models) != len(self.group.models) or not R <= n <= _lib.TOPK_MAX_N:
            raise _lib.MobocmfError("DeviceAcqSearch: the raw candidates in equal chunks of the raw group's T test points")
        if (n, Tc) not in self._raw:
            dev = self.group.device
            self._raw[(n, Tc)] = (torch.zeros(B, n, dtype=torch.float64, device=dev), torch.zeros(B, R, dtype=torch.float64, device=dev),
                                  torch.zeros(B, R, dtype=torch.int64, device=dev), raw_group.noise().detach().clone().contiguous(),
                                  torch.zeros(n, self.d, dtype=torch.float64, device=dev))
        vals, top_v, top_i, noise, xraw = self._raw[(n, Tc)]
        self.raw_group, self.raw_values = raw_group, self._one(vals)
        raw_group.freeze()
        xraw.copy_(Xraw.detach().reshape(n, self.d))
        for c in range(n // Tc):
            raw_group.x.copy_(xraw[c * Tc:(c + 1) * Tc])
            raw_group._launch(_lib.STEP_FORWARD)
            self._jes(raw_group, noise, vals[:, c * Tc:(c + 1) * Tc])
        for p in range(B):
            F.select_topk(vals[p], R, top_v[p], top_i[p], x=xraw, out_x=self.group.x[p * R:(p + 1) * R], stream=self.group.stream)
        return self._one(vals), self._one(top_v), self._one(top_i)

    def run(self, x0=None, maxiter=200):
        """``x0`` (num_restarts, d): the starting points (None: what ``start_from_raw`` left in the group's x)."""
        g = self.group
        maxiter = int(maxiter)
        with torch.no_grad(), self._stream_ctx():
            if x0 is not None:
                g.x.copy_(x0.detach().reshape(self.T, self.d))
            self.best_v.fill_(float("-inf"))
            self.exp_avg.zero_()
            self.exp_avg_sq.zero_()
            self.steps_done.zero_()
            g.freeze()
            left = maxiter
            if left > 0:
                self._iterate()
                left -= 1
            if self.use_graph:
                per = max(1, int(self.iters_per_graph))
                for n, times in ((per, left // per), (1, left % per)):
                    if times:
                        graph = self._graph(n)
                        for _ in range(times):
                            graph.replay()
            else:
                for _ in range(left):
                    self._iterate()
            self._score(seeds=False)      # X_maxiter
            return self._winner()

    def _winner(self):
        """Per search the best of its restarts' best iterates: (candidates (B, d), values (B,) -- coupled: ()), device tensors."""
        R = self.R
        for p in range(self.B):
            F.select_topk(self.best_v[p * R:(p + 1) * R], 1, self.win_v[p:p + 1], self.win_i[p:p + 1],
                          x=self.best_x[p * R:(p + 1) * R], out_x=self.cand[p:p + 1], stream=self.group.stream)
        return self.cand.clone(), self._one(self.win_v).clone()

    def info_words(self):
        """The Cholesky verdicts of the models of the search group and of the raw-candidate group last used (int32 words, 0:
        fine) as one device tensor; no synchronisation."""
        raw = self.__dict__.get("raw_group")
        return torch.cat([w.reshape(-1) for g in (self.group, raw) if g is not None for w in g.info_words])


class DecoupledDeviceAcqSearch(DeviceAcqSearch):
    """The searches of ALL black-boxes of a fidelity at once, each for its own JES term (decoupled evaluations:
    JESMOC_MFDGP.get_nextpoint_decoupled).  ``group``: an ordinary predict group over the B (1 + K) models, built for
    T = B R test points (R = ``num_restarts``); rows [p R, (p + 1) R) of its x are the restarts of black-box p.  An iterate is
    the same chain of four launches with mobocmf_jes_mc_box_forward in selected-box mode in place of the coupled JES launch:
    it seeds the models of a row's own box and writes ZERO seeds for every other model, so mobocmf_ascent_adam_step's sum of gx
    over all models is the gradient of the row's own term.  Every model is therefore evaluated at all B R rows though only R
    are its own.

    Only the JES launch differs from the coupled engine (``_jes``): ``start_from_raw`` scores the raw candidates ONCE for all
    boxes (the forward launches of the coupled search, then the all-box mode into ``vals`` (B, n)) and picks each box's R
    best.  ``run`` -> (candidates (B, d), values (B,)), device tensors, without synchronising."""

    def __init__(self, group, bounds, num_restarts, lr, betas=(0.9, 0.999), eps=1e-8, num_pareto_samples=1):
        K, R = int(num_pareto_samples), int(num_restarts)
        if K < 1 or R < 1:
            raise ValueError("DecoupledDeviceAcqSearch: num_pareto_samples >= 1 and num_restarts >= 1 (got %d, %d)" % (K, R))
        n_models = len(group.models)
        B = n_models // (1 + K)
        if n_models % (1 + K) or B < 1 or group.T != B * R:
            raise _lib.MobocmfError("DecoupledDeviceAcqSearch: a group of (uncond, cond_1 .. cond_K) per black-box built for T = "
                                    "(black-boxes) x num_restarts test points")
        if B * R > _lib.TOPK_MAX_N or B * (1 + K) > 2 * _lib.ACQ_MAX_PAIRS:
            raise _lib.MobocmfError("DecoupledDeviceAcqSearch: at most %d rows and %d models" % (_lib.TOPK_MAX_N, 2 * _lib.ACQ_MAX_PAIRS))
        super().__init__(group, bounds, R, lr, betas=betas, eps=eps, num_pareto_samples=K, n_searches=B)
        self.box_of_point = torch.div(torch.arange(B * R, device=group.device), R, rounding_mode="floor").to(torch.int32).contiguous()

    def _jes(self, grp, noise, acq, **track):
        """An iterate: every row for the box it is searched for; a chunk of raw candidates: every box's term at every row."""
        F.jes_mc_box_forward(grp.moments, noise, self.K, grp.T, grp.S, acq, box_of_point=self.box_of_point if track else None,
                             stream=grp.stream, **track)


class MesDeviceAcqSearch(DeviceAcqSearch):
    """The coupled MES search of the exact-GP baseline (``MESMOC_MFGP(search="device")``): ``group`` is an ExactGPPredictGroup
    (util/exact_predict.py) over the ``n_obj`` objectives' models, then the ``n_con`` constraints' models, built for T =
    ``num_restarts`` test points; ``best`` (n_obj + n_con,): best value per objective, threshold per constraint.  The iterate is
    the same chain of four launches -- group STEP_FORWARD -> mobocmf_mes_group_forward -> group STEP_INPUT_GRADIENTS ->
    mobocmf_ascent_adam_step -- captured once and replayed; ``start_from_raw``, ``run`` and the winner are the base class's."""

    def __init__(self, group, bounds, num_restarts, lr, best, n_obj, n_con, betas=(0.9, 0.999), eps=1e-8):
        self.n_obj, self.n_con = int(n_obj), int(n_con)
        super().__init__(group, bounds, num_restarts, lr, betas=betas, eps=eps)
        self.best = torch.as_tensor(best, dtype=torch.float64).detach().reshape(-1).to(group.device).contiguous()
        if self.best.numel() != self.n_obj + self.n_con:
            raise _lib.MobocmfError("MesDeviceAcqSearch: one best value per objective and one threshold per constraint")

    def _check_group(self, group):
        if group.T != self.R or group.S != 1:
            raise _lib.MobocmfError("MesDeviceAcqSearch: a group with S = 1 built for T = num_restarts test points")
        if self.n_obj < 1 or self.n_con < 0 or len(group.models) != self.n_obj + self.n_con or \
                len(group.models) > 2 * _lib.ACQ_MAX_PAIRS:
            raise _lib.MobocmfError("MesDeviceAcqSearch: n_obj >= 1 objectives then n_con >= 0 constraints, at most %d models"
                                    % (2 * _lib.ACQ_MAX_PAIRS))

    def _jes(self, grp, noise, acq, **track):
        """The MES launch in the JES position (``acq`` (T,) of an iterate, or (1, chunk) of raw candidates)."""
        F.mes_group_forward(grp.moments, noise, self.best, self.n_obj, self.n_con, grp.T, acq, stream=grp.stream, **track)


def raise_on_info(words, what):
    """``words``: HOST int32 info words of one-launch models (0: fine; > 0: the failed pivot; < 0: an abandoned in-launch wait)."""
    from ..layers.mfdgp_hidden_layer import NotPSDError
    bad = [int(v) for v in words.reshape(-1).tolist() if int(v) != 0]
    if bad:
        if bad[0] < 0:
            raise F.InLaunchWaitAbandoned("%s: in-launch barrier abandoned (info %d)" % (what, bad[0]))
        raise NotPSDError("%s: K_mm not positive definite (pivot %d)" % (what, bad[0]))
