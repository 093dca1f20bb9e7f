"""JES acquisition on MFDGP surrogates -- host mirror of mobocmf/acquisition_functions/JESMOC_MFDGP.py
(``_JES_MFDGP.forward`` :38-52, ``JESMOC_MFDGP`` :55-184).

The per-black-box value 0.5 * clamp(log v_uncond - log v_cond, 0) runs on the HIP path (predict_for_acquisition of
both models + functional.jes) and is differentiable w.r.t. X.  botorch's ``optimize_acqf`` (absent here, SURVEY row
N3) is replaced by ``optimize_acqf_multistart``: the same recipe -- ``raw_samples`` uniform candidates, the best
``num_restarts`` refined by projected gradient ascent (Adam) for ``maxiter`` steps, ALL restarts in one batch so every
iteration is a single pair of model evaluations.  With surrogates sharded over ranks the coupled acquisition is the
all-gather + sum of mobocmf_amd.parallel.coupled_acquisition.

``JESMOC_MFDGP(search="device")``: wherever the black-boxes of a fidelity fit a one-launch predict group (M <= 128) or the
frozen-chain predict groups (128 < M <= 1024, util/panel_predict.py) the whole search -- scoring of the raw candidates, choice of
the restarts, the ascent, the best iterate, the final pick -- runs on the GPU (util/acq_search.py DeviceAcqSearch,
csrc/acq_search.hip), one graph replay per iterate, and the host reads the device once per ``get_nextpoint_coupled`` call.

``get_nextpoint_decoupled`` answers which black-box to evaluate next: every black-box's own JES term is maximised from one draw
of raw candidates and weighed by that black-box's cost (the reference has ``decoupled_acq`` :118-123 and nothing that maximises
it); with ``search="device"`` all black-boxes of a fidelity are searched at once (DecoupledDeviceAcqSearch).
"""
import contextlib

import torch

from .. import functional as F
from .. import parallel


class _JES_MFDGP:
    """JES of one black-box at one fidelity.  ``mfdgp_cond``: the conditioned model, or a list of K models conditioned on K
    sampled Pareto sets: the value is then the mean of the K single-sample values (the Monte Carlo estimate of the information
    gain), the unconditioned model evaluated once.  ``mfdgp_conds`` is the list, ``mfdgp_cond`` its first."""

    def __init__(self, fidelity, mfdgp_uncond, mfdgp_cond, model=None):
        assert model is None
        self.fidelity = fidelity
        self.mfdgp_uncond = mfdgp_uncond
        self.mfdgp_conds = list(mfdgp_cond) if isinstance(mfdgp_cond, (list, tuple)) else [mfdgp_cond]
        if not self.mfdgp_conds:
            raise ValueError("_JES_MFDGP: at least one conditioned model")
        self.mfdgp_cond = self.mfdgp_conds[0]

    def forward(self, X):
        """Evaluate JES at X (T, d) or (T, 1, d).  The models are switched to ``.eval()`` (full predictive branch,
        no clamp) exactly as the reference does (:42-50).  K > 1: (1/K) sum_k 0.5 clamp(log v_u - log v_c,k, 0), summed in the
        order of k."""
        self.mfdgp_uncond.eval()
        _, v_u = self.mfdgp_uncond.predict_for_acquisition(X, self.fidelity)
        self.mfdgp_uncond.train()
        total = None
        for cond in self.mfdgp_conds:
            cond.eval()
            _, v_c = cond.predict_for_acquisition(X, self.fidelity)
            cond.train()
            term = F.jes(v_u, v_c)
            total = term if total is None else total + term
        K = len(self.mfdgp_conds)
        return total if K == 1 else (1.0 / K) * total

    __call__ = forward

    @contextlib.contextmanager
    def frozen(self):
        """All models' parameters are constants while the acquisition is optimised: their M x M chains are computed
        once (MFDGP.frozen_chains) instead of at each of the ~400 evaluations."""
        with contextlib.ExitStack() as stack:
            for m in [self.mfdgp_uncond] + self.mfdgp_conds:
                stack.enter_context(m.frozen_chains())
            yield self


def optimize_acqf_multistart(acq_function, bounds, num_restarts=5, raw_samples=200, maxiter=200, lr=0.02,
                             generator=None, Xraw=None):
    """Maximise ``acq_function`` over the box ``bounds`` (2, d).  Returns (candidate (1, d), value).  ``Xraw`` (n, d): the raw
    candidates to start from, in place of the draw of ``raw_samples`` uniform ones (several searches from the same candidates)."""
    lo, hi = bounds[0], bounds[1]
    d = lo.numel()
    dev, dt = lo.device, lo.dtype
    with torch.no_grad():
        if Xraw is None:
            Xraw = lo + (hi - lo) * torch.rand(raw_samples, d, dtype=dt, device=dev, generator=generator)
        else:
            Xraw, raw_samples = Xraw.detach().clone(), Xraw.shape[0]
        parallel.broadcast_(Xraw)     # sharded surrogates: every rank scores (and all-gathers values of) the same points
        vals = acq_function(Xraw)
        X = Xraw[torch.topk(vals, min(num_restarts, raw_samples)).indices].clone()
    X.requires_grad_(True)
    if X.is_cuda and X.dtype == torch.float64:
        # the library's one-launch Adam (torch.optim.Adam's update; also spares the process the ~0.6 s of lazy imports that
        # the first torch.optim step pulls in -- more than a whole search at the reference's sizes)
        opt = F.FusedAdam([X], lr=lr * float((hi - lo).mean()))
    else:
        opt = torch.optim.Adam([X], lr=lr * float((hi - lo).mean()))
    # every iterate X_0 ... X_maxiter is scored ONCE: the value of the evaluation that also yields its gradient is the score of the
    # iterate (round 4 scored X_{t+1} after the step and evaluated it again, with gradient, at the top of the next iteration --
    # a third of the search's launches)
    best_x, best_v = X.detach().clone(), None
    for it in range(maxiter + 1):
        last = it == maxiter
        opt.zero_grad()
        if last:
            with torch.no_grad():
                v = acq_function(X)
        else:
            v = acq_function(X)
        with torch.no_grad():
            vd = v.detach()
            if best_v is None:
                best_v = vd.clone()
            else:
                better = vd > best_v
                best_v = torch.where(better, vd, best_v)
                best_x[better] = X.detach()[better]
        if last:
            break
        (-v.sum()).backward()
        opt.step()
        with torch.no_grad():
            X.clamp_(min=lo, max=hi)
            parallel.broadcast_(X)    # (no-op on one rank) summation order may differ by an ulp between ranks
    k = int(torch.argmax(best_v))
    return best_x[k:k + 1].detach(), best_v[k].detach()


def _read_once(vals, words=None):
    """ONE device-to-host copy of the float64 values ``vals`` (n,) and the int32 ``words`` (or None): the words are padded to
    an even count and reinterpreted -- not converted -- as float64, two to a double, appended to the values, copied, and
    reinterpreted back on the host.  A copy keeps every bit, whatever NaN pattern two words happen to spell.  Returns host
    tensors (values, words or None)."""
    if words is None:
        return vals.cpu(), None
    n, k = vals.numel(), words.numel()
    padded = torch.cat([words.reshape(-1).to(torch.int32), words.new_zeros(k % 2, dtype=torch.int32)])
    host = torch.cat([vals.reshape(-1), padded.view(torch.float64)]).cpu()
    return host[:n], host[n:].view(torch.int32)[:k]


class JESMOC_MFDGP:

    search = "host"           # "device": the search itself on the GPU wherever a one-launch predict group fits (_optimize)
    num_pareto_samples = 1    # (class defaults: what an object made with __new__ has)
    _search_running = False   # inside _frozen_groups(): coupled_acq freezes the group it evaluates through
    blackbox_mfdgp_fitters_cond = None
    num_restarts, raw_samples, search_lr = 5, 200, 0.02      # the recipe of both engines
    MAX_RAW_CHUNKS = 8        # the device engine scores the raw candidates in at most this many forward launches

    def __init__(self, model, num_fidelities=1, model_cond=None, standard_bounds=None, eval_highest_fidelity=False,
                 search="host", num_pareto_samples=1, pareto_seed=None):
        """``num_pareto_samples`` = K: the acquisition is the average of JES over K sampled Pareto sets, each with its own
        conditioned fit (BlackBoxMFDGPFitter.conditioned_copies; ``pareto_seed``: the seeded sampling procedure, sample k from a
        seed derived from (pareto_seed, k), sample 0 from pareto_seed itself).  ``model_cond``: a conditioned fitter, or a
        list / tuple of K of them (``num_pareto_samples`` is then their number).  K = 1 is the reference's estimator."""
        if search not in ("host", "device"):
            raise ValueError("search must be 'host' or 'device' (got %r)" % (search,))
        conds = None if model_cond is None else (list(model_cond) if isinstance(model_cond, (list, tuple)) else [model_cond])
        K = int(num_pareto_samples) if conds is None else len(conds)
        if K < 1:
            raise ValueError("num_pareto_samples must be >= 1 (got %r)" % (num_pareto_samples,))
        if K > 1 and not parallel._no_group():
            raise ValueError("num_pareto_samples = %d: several Pareto samples are limited to one process (surrogates sharded "
                             "over a process group take num_pareto_samples = 1)" % K)
        self.num_pareto_samples = K
        self.search = search
        self.last_search_engine = {}      # fidelity -> "host" / "device": the engine its last search ran on
        self.standard_bounds = standard_bounds
        self.eval_highest_fidelity = eval_highest_fidelity
        self.blackbox_mfdgp_fitter_uncond = model.copy_uncond()
        if conds is None:
            # reference (:64-66): sample a Pareto solution (RFF posterior samples + MOOP) unless one was provided; K > 1: K of them
            conds = model.conditioned_copies(K, seed=pareto_seed)
            self.samples_objs, self.samples_cons = getattr(model, "samples_objs", None), getattr(model, "samples_cons", None)
        self.blackbox_mfdgp_fitters_cond = conds
        self.pareto_sets, self.pareto_fronts = [c.pareto_set for c in conds], [c.pareto_front for c in conds]
        self.pareto_set, self.pareto_front = self.pareto_sets[0], self.pareto_fronts[0]      # (sample 0, as ever)
        self.blackbox_mfdgp_fitter_cond = conds[0]
        self.num_fidelities = num_fidelities
        self.objectives, self.constraints, self.costs_blackboxes = {}, {}, {}
        for n_f in range(num_fidelities):
            self.objectives[n_f] = {}
            self.constraints[n_f] = {}
            self.costs_blackboxes[n_f] = {"total": 0.0}

    def add_blackbox(self, fidelity, blackbox_name, cost_evaluation=1.0, is_constraint=False):
        """Registers a black-box's acquisition at ``fidelity`` and adds its cost to the fidelity's total.  Black-boxes
        sharded over ranks: every rank adds EVERY black-box, so that all ranks weigh the fidelities by the same totals; a
        black-box another rank holds only has its cost recorded here (returns None)."""
        held = self.blackbox_mfdgp_fitter_uncond.mfdgp_handlers_cons if is_constraint else \
            self.blackbox_mfdgp_fitter_uncond.mfdgp_handlers_objs
        if blackbox_name not in held and not parallel._no_group():
            self.costs_blackboxes[fidelity]["total"] += cost_evaluation
            self.costs_blackboxes[fidelity][blackbox_name] = cost_evaluation
            return None
        mfdgp_uncond = self.blackbox_mfdgp_fitter_uncond.get_model(blackbox_name, is_constraint=is_constraint)
        fitters_cond = self.blackbox_mfdgp_fitters_cond or [self.blackbox_mfdgp_fitter_cond]
        mfdgp_conds = [c.get_model(blackbox_name, is_constraint=is_constraint) for c in fitters_cond]
        jes_mfdgp = _JES_MFDGP(fidelity, mfdgp_uncond, mfdgp_conds if len(mfdgp_conds) > 1 else mfdgp_conds[0])
        (self.constraints if is_constraint else self.objectives)[fidelity][blackbox_name] = jes_mfdgp
        self.costs_blackboxes[fidelity]["total"] += cost_evaluation
        self.costs_blackboxes[fidelity][blackbox_name] = cost_evaluation
        return jes_mfdgp

    def decoupled_acq(self, X, fidelity, blackbox_name, is_constraint=True):
        d = self.constraints if is_constraint else self.objectives
        return d[fidelity][blackbox_name](X.double())

    use_tiny_step = True      # False: always the layer path (A/B, tests)

    def __getstate__(self):
        state = self.__dict__.copy()
        state.pop("_tiny_groups", None)      # device descriptors: rebuilt on first use
        state.pop("_panel_groups", None)
        state.pop("_device_searches", None)  # ... and the captured graphs over them
        state.pop("_decoupled_searches", None)
        return state

    @staticmethod
    def _group_models(jess):
        """The model list of a predict group: per black-box its unconditioned surrogate, then the K conditioned ones."""
        return [m for jes in jess for m in [jes.mfdgp_uncond] + jes.mfdgp_conds]

    def _box_values(self, v):
        """Every black-box's own term from a group's v (n_boxes (1 + K), T): row p = (1/K) sum_k 0.5 clamp(log v_u,p - log v_c,pk, 0),
        the k-sum in the order of k (mobocmf_jes_mc_box_forward's term_p).  K = 1: 1.0 * the single term is exact."""
        K = self.num_pareto_samples
        lu = torch.log(v[0::1 + K])
        box = None
        for k in range(1, K + 1):
            term = 0.5 * torch.clamp(lu - torch.log(v[k::1 + K]), min=0.0)
            box = term if box is None else box + term
        return (1.0 / K) * box

    def _group_value(self, v):
        """The coupled acquisition from a group's v: the sum of ``_box_values`` over the black-boxes (the expression of
        mobocmf_jes_mc_group_forward)."""
        return self._box_values(v).sum(0)

    def _group_box_value(self, v, p):
        """Black-box p's own term from a group's v: the summand of ``_group_value``."""
        return self._box_values(v)[p]

    def _group_v(self, X, fidelity):
        """v (n_boxes (1 + K), T) of every model of ``fidelity`` at X (float64) through the one-launch predict group, where the
        acquisition is evaluated through one (small surrogates on the GPU, one process); else None: the layer path."""
        jess = [j for _, _, j in self._boxes(fidelity)]
        if self.use_tiny_step and jess and X.is_cuda and parallel.world()[1] == 1:
            X2 = X[:, 0, :] if X.dim() > 2 else X
            grp = self._tiny_group(jess, fidelity, X2.shape[0], X2.shape[1])
            if grp is not None:
                if self._search_running:
                    grp.freeze()      # (constant parameters for the whole search: the chains are formed by its first launch only)
                return grp.acquisition_moments(X2)[1]
        return None

    def _first_group(self, classes, jess, fidelity, T, d, speed_rule=(), **kw):
        """A predict group (util/predict_group.py) over (uncond, cond_1 .. cond_K) of every black-box in ``jess`` for T test
        points, of the first of ``classes`` whose ``why_not`` is None for every model (for a class in ``speed_rule``: with its
        speed rule on); None where none fits or the models are not on the GPU.  ``kw``: further constructor arguments.  With
        several Pareto samples a group that its constructor refuses (MobocmfError) is no group either; with one it raises."""
        from .._lib import MobocmfError
        models = self._group_models(jess)
        if not (models and all(p.is_cuda for p in models[0].parameters())):
            return None
        for cls in classes:
            gate = dict(speed_rule=True) if cls in speed_rule else {}
            if all(cls.why_not(m, fidelity, T, d, **gate) is None for m in models):
                try:
                    return cls(models, fidelity, T, d, **kw)
                except MobocmfError:
                    if self.num_pareto_samples == 1:
                        raise
                    return None
        return None

    def _tiny_group(self, jess, fidelity, T, d):
        """TinyPredictGroup (M <= 32, where one workgroup beats the layer path) or CoopPredictGroup (M <= 128: the cooperative
        launch, several workgroups per model) when all models fit a one-launch kernel (util/tiny_step.py, util/coop_step.py) --
        else None.  Built once per (fidelity, T, d)."""
        cache = self.__dict__.setdefault("_tiny_groups", {})
        key = (fidelity, T, d)
        if key not in cache:
            from ..util.coop_step import CoopPredictGroup
            from ..util.tiny_step import TinyPredictGroup
            cache[key] = self._first_group((TinyPredictGroup, CoopPredictGroup), jess, fidelity, T, d, speed_rule=(TinyPredictGroup,))
        return cache[key]

    def _panel_group(self, jess, fidelity, T, d, want_gradients):
        """PanelPredictGroup (128 < M <= 512, util/panel_predict.py) when all models fit; else SplitPredictGroup (M <= 1024:
        8-column panels, replicas split over workgroups) when all of them fit that; else None.  A cache of the DEVICE engine
        alone: ``coupled_acq`` never looks here, so the host engine evaluates these sizes through the layer path as ever."""
        cache = self.__dict__.setdefault("_panel_groups", {})
        key = (fidelity, T, d, bool(want_gradients))
        if key not in cache:
            from ..util.panel_predict import PanelPredictGroup, SplitPredictGroup
            cache[key] = self._first_group((PanelPredictGroup, SplitPredictGroup), jess, fidelity, T, d, want_gradients=want_gradients)
        return cache[key]

    def coupled_acq(self, X, fidelity):
        """Sum over all black-boxes (:125-135).  Sharded surrogates: each rank adds its own, one all-gather sums.
        Small surrogates (the reference's own sizes): the predictive moments of ALL models -- unconditioned and conditioned,
        every black-box -- come from one launch, their gradient w.r.t. X from one more (TinyPredictGroup); the JES value
        0.5 clamp(log v_uncond - log v_cond, 0) (:38-52) is then a handful of element-wise operations over all of them.
        With K > 1 sampled Pareto sets the value of a black-box is the mean over its K conditioned surrogates (_group_value)."""
        X = X.double()
        v = self._group_v(X, fidelity)
        if v is not None:
            return self._group_value(v)
        local = [obj(X) for obj in self.objectives[fidelity].values()] + \
                [con(X) for con in self.constraints[fidelity].values()]
        if not local:
            local = [torch.zeros(X.shape[0], dtype=X.dtype, device=X.device)]
        acq = torch.stack(local).sum(0)
        _, w = parallel.world()
        if w > 1:       # every rank enters the exchange, also one that holds no black-box of this fidelity
            acq = acq + (parallel.coupled_acquisition(acq.detach()[None]) - acq.detach())
        return acq

    @contextlib.contextmanager
    def _frozen_groups(self):
        """The one-launch predict groups used inside keep their chains (util/coop_step.py CoopPredictGroup.freeze)."""
        self._search_running = True
        try:
            yield
        finally:
            self._search_running = False
            failed = None      # every group is thawed, also after one of them reported an abandoned wait
            groups = list(self.__dict__.get("_tiny_groups", {}).values()) + list(self.__dict__.get("_panel_groups", {}).values())
            for grp in groups:
                if grp is not None:
                    try:
                        grp.thaw()
                    except F.InLaunchWaitAbandoned as e:
                        failed = failed or e
            if failed is not None:
                raise failed

    def _routed_search(self, fidelity, n_searches, engine_cls, cache_name):
        """(engine, raw-candidate group) of ``fidelity`` when its ``n_searches`` searches of num_restarts rows each (None: the one
        coupled search) can stay on the GPU -- the condition under which ``coupled_acq`` evaluates through a one-launch group, and a group fits
        T = n_searches x num_restarts and the raw candidates, whole or in up to ``MAX_RAW_CHUNKS`` equal chunks (200 candidates
        x 25 samples are beyond the kernels' 4096 columns); or, where no one-launch group fits, frozen-chain groups do
        (128 < M <= 1024: the raw candidates whole, no column limit there) -- else None: M > 1024, S = 1, sharded surrogates,
        CPU tensors keep the host loop.  A group holds 1 + K models per black-box: more than 2 MOBOCMF_ACQ_MAX_PAIRS models or
        MOBOCMF_TOPK_MAX_N rows keep the host loop too (the coupled search at K = 1 leaves that to the group's constructor, as
        ever).  ``engine_cls`` (util/acq_search.py) is built once per fidelity and group in the cache ``cache_name``."""
        from .. import _lib
        jess = [j for _, _, j in self._boxes(fidelity)]
        bounds = self.standard_bounds
        if not (self.use_tiny_step and jess and bounds is not None and bounds.is_cuda and parallel.world()[1] == 1):
            return None
        K, R = self.num_pareto_samples, self.num_restarts
        rows = (n_searches or 1) * R
        if (K > 1 or n_searches) and len(jess) * (1 + K) > 2 * _lib.ACQ_MAX_PAIRS:
            return None
        if R > self.raw_samples or (n_searches and rows > _lib.TOPK_MAX_N):
            return None
        d = bounds.shape[1]
        grp = self._tiny_group(jess, fidelity, rows, d)
        if grp is None:
            grp = self._panel_group(jess, fidelity, rows, d, True)
            raw = None if grp is None else self._panel_group(jess, fidelity, self.raw_samples, d, False)
        else:
            chunks = [c for c in range(1, self.MAX_RAW_CHUNKS + 1) if self.raw_samples % c == 0]
            raw = next((g for g in (self._tiny_group(jess, fidelity, self.raw_samples // c, d) for c in chunks) if g is not None),
                       None)
        if raw is None:
            return None
        cache = self.__dict__.setdefault(cache_name, {})
        if fidelity not in cache or cache[fidelity].group is not grp:
            cache[fidelity] = engine_cls(grp, bounds, R, self.search_lr, num_pareto_samples=K)
        return cache[fidelity], raw

    def _device_search(self, fidelity):
        """(DeviceAcqSearch, raw-candidate group) of the coupled search of ``fidelity``, or None: the host engine."""
        from ..util.acq_search import DeviceAcqSearch
        return self._routed_search(fidelity, None, DeviceAcqSearch, "_device_searches")

    def _search(self, fidelity, maxiter, generator, decoupled):
        """[(candidate (1, d), value)] of the searches at ``fidelity`` from ONE draw of raw candidates: the coupled search, or
        (``decoupled``) every black-box's own term in the order of ``_boxes``.  ``self.last_search_engine[fidelity]`` says where
        they ran."""
        if self.search not in ("host", "device"):
            raise ValueError("search must be 'host' or 'device' (got %r)" % (self.search,))
        engines = self.__dict__.setdefault("last_search_engine", {})
        boxes = self._boxes(fidelity)
        with contextlib.ExitStack() as stack:       # fitted models: freeze every surrogate's chain for the whole search
            for _, _, jes in boxes:
                stack.enter_context(jes.frozen())
            stack.enter_context(self._frozen_groups())      # (its exit thaws the groups: an abandoned in-launch wait raises there)
            route = self._decoupled_device_search if decoupled else self._device_search
            found = route(fidelity) if self.search == "device" else None
            lo, hi = self.standard_bounds[0], self.standard_bounds[1]
            with torch.no_grad():      # the draw of optimize_acqf_multistart: both engines see the same points
                Xraw = lo + (hi - lo) * torch.rand(self.raw_samples, lo.numel(), dtype=lo.dtype, device=lo.device,
                                                   generator=generator)
                if found is not None:
                    engine, raw = found
                    engine.start_from_raw(raw, Xraw)
                    engines[fidelity] = "device"
                    cands, vals = engine.run(None, maxiter)
                    return [(cands[p:p + 1], v) for p, v in enumerate(vals.reshape(-1))]
            engines[fidelity] = "host"
            if decoupled:
                acqs = [lambda x, p=p, name=name, con=con: self._box_acq(x, fidelity, p, name, con)
                        for p, (name, con, _) in enumerate(boxes)]
            else:
                acqs = [lambda x: self.coupled_acq(x, fidelity=fidelity)]
            return [optimize_acqf_multistart(fn, self.standard_bounds, num_restarts=self.num_restarts, raw_samples=self.raw_samples,
                                             maxiter=maxiter, lr=self.search_lr, Xraw=Xraw) for fn in acqs]

    def _optimize(self, fidelity, **kw):
        """(candidate (1, d), value) of the coupled search at ``fidelity``."""
        return self._search(fidelity, kw.get("maxiter", 200), kw.get("generator"), False)[0]

    def _get_nextpoint_coupled_highest_fidelity(self, iteration=None, verbose=False, maxiter=200, generator=None):
        """Reference name (:137-149): search the highest fidelity only."""
        keep, self.eval_highest_fidelity = self.eval_highest_fidelity, True
        try:
            return self.get_nextpoint_coupled(iteration=iteration, verbose=verbose, maxiter=maxiter, generator=generator)
        finally:
            self.eval_highest_fidelity = keep

    def _get_nextpoint_coupled(self, iteration=None, verbose=False, maxiter=200, generator=None):
        """Reference name (:151-176): search every fidelity, pick the best cost-weighted value."""
        keep, self.eval_highest_fidelity = self.eval_highest_fidelity, False
        try:
            return self.get_nextpoint_coupled(iteration=iteration, verbose=verbose, maxiter=maxiter, generator=generator)
        finally:
            self.eval_highest_fidelity = keep

    def _pick_on_host(self, found, cache_name):
        """``found``: [(candidate, value, cost, key)], key = (fidelity, ...), with the winners still on the device.  ONE read
        fetches them all and the info words of every model the device engines of ``cache_name`` ran; the weighting and the
        choice are the arithmetic of the loop in ``get_nextpoint_coupled`` on host doubles (the largest value / cost, ties to
        the earlier).  Returns ((w, candidate, key), {key: value})."""
        from ..util.acq_search import raise_on_info
        vals = torch.stack([v.detach().reshape(()).double() for _, v, _, _ in found])
        searches = self.__dict__.get(cache_name, {})
        ran = [f for f in dict.fromkeys(key[0] for _, _, _, key in found) if self.last_search_engine.get(f) == "device"]
        infos = [searches[f].info_words() for f in ran]
        host, words = _read_once(vals, torch.cat(infos) if infos else None)
        if words is not None:
            raise_on_info(words, "device acquisition search")
        best = None
        for k, (cand, _, cost, key) in enumerate(found):
            w = float(host[k]) / cost
            if best is None or best[0] < w:
                best = (w, cand, key)
        return best, {key: float(host[k]) for k, (_, _, _, key) in enumerate(found)}

    def get_nextpoint_coupled(self, iteration=None, verbose=False, maxiter=200, generator=None):
        """Next point + fidelity by cost-weighted acquisition (:137-184).  ``generator``: the raw candidates' draw."""
        fids = [self.num_fidelities - 1] if self.eval_highest_fidelity else list(range(self.num_fidelities))
        best, found = None, []
        for fidelity in fids:
            cand, val = self._optimize(fidelity, maxiter=maxiter, generator=generator)
            cost = self.costs_blackboxes[0 if self.eval_highest_fidelity else fidelity]["total"]
            if self.search == "device":      # the winners stay on the device until every fidelity is done
                found.append((cand, val, cost, (fidelity,)))
                continue
            w = val / cost
            if best is None or best[0] < w:
                best = (w, cand, (fidelity,))
        if found:
            best, values = self._pick_on_host(found, "_device_searches")
            self.last_search_values = {f: v for (f,), v in values.items()}
        w, cand, (fidelity,) = best
        if not parallel._no_group():     # sharded: every rank returns rank 0's choice (ties may break by an ulp)
            dec = torch.cat([cand.reshape(-1).detach().double(), torch.tensor([float(fidelity)], dtype=torch.float64,
                                                                             device=cand.device)])
            parallel.broadcast_(dec, 0)
            cand, fidelity = dec[:-1].reshape(cand.shape).to(cand.dtype), int(dec[-1])
        if verbose:
            print("Iter:", iteration, "Acquisition:", float(w * self.costs_blackboxes[fidelity]["total"]),
                  " Evaluating fidelity", fidelity, "at", cand[0].cpu().numpy())
        return cand[0, :], fidelity

    # ------------------------------------------------------------------ decoupled evaluations: which black-box next
    def _boxes(self, fidelity):
        """[(name, is_constraint, jes)] of ``fidelity``: objectives, then constraints, in insertion order -- the order of the
        models in a predict group (``_device_search``), so the position in this list is the box index p."""
        return [(n, False, j) for n, j in self.objectives[fidelity].items()] + \
               [(n, True, j) for n, j in self.constraints[fidelity].items()]

    def _box_acq(self, X, fidelity, p, blackbox_name, is_constraint):
        """Black-box p's own term at X: through the predict group ``coupled_acq`` would evaluate through, else ``decoupled_acq``."""
        X = X.double()
        v = self._group_v(X, fidelity)
        if v is not None:
            return self._group_box_value(v, p)
        return self.decoupled_acq(X, fidelity, blackbox_name, is_constraint=is_constraint)

    def _decoupled_device_search(self, fidelity):
        """(DecoupledDeviceAcqSearch, raw-candidate group) under the routing of ``_device_search``, the search group built for
        (black-boxes) x num_restarts test points; None: the host engine.  Cached apart from the coupled searches."""
        from ..util.acq_search import DecoupledDeviceAcqSearch
        return self._routed_search(fidelity, len(self._boxes(fidelity)), DecoupledDeviceAcqSearch, "_decoupled_searches")

    def _optimize_decoupled(self, fidelity, maxiter=200, generator=None):
        """[(candidate (1, d), value)] per black-box of ``fidelity`` in the order of ``_boxes``: every box's own term maximised
        from ONE draw of raw candidates (the draw of ``_optimize``)."""
        return self._search(fidelity, maxiter, generator, True)

    def get_nextpoint_decoupled(self, iteration=None, verbose=False, maxiter=200, generator=None):
        """Which black-box to evaluate next, where and at which fidelity: every registered (fidelity, black-box) has its own JES
        term maximised (``search``: on the host, or all black-boxes of a fidelity at once on the GPU), the value is weighed by
        1 / costs_blackboxes[fidelity][name], the largest wins, ties to the earlier (fidelity, black-box).  Returns
        (x (d,), fidelity, blackbox_name, is_constraint); ``last_decoupled_values[(fidelity, name)]``: the unweighted values."""
        if not parallel._no_group():
            raise ValueError("get_nextpoint_decoupled is limited to one process (surrogates sharded over a process group have "
                             "get_nextpoint_coupled)")
        fids = [self.num_fidelities - 1] if self.eval_highest_fidelity else list(range(self.num_fidelities))
        found = []
        for fidelity in fids:
            boxes = self._boxes(fidelity)
            if not boxes:
                continue
            res = self._optimize_decoupled(fidelity, maxiter=maxiter, generator=generator)
            found += [(cand, val, self.costs_blackboxes[fidelity][name], (fidelity, name, con))
                      for (cand, val), (name, con, _) in zip(res, boxes)]
        if not found:
            raise ValueError("get_nextpoint_decoupled: no black-box registered (add_blackbox)")
        (w, cand, (fidelity, name, con)), values = self._pick_on_host(found, "_decoupled_searches")      # the one read of the device
        self.last_decoupled_values = {(f, n): v for (f, n, _), v in values.items()}
        if verbose:
            print("Iter:", iteration, "Acquisition:", float(w * self.costs_blackboxes[fidelity][name]), " Evaluating",
                  "constraint" if con else "objective", name, "at fidelity", fidelity, "at", cand[0].cpu().numpy())
        return cand[0, :], fidelity, name, con
