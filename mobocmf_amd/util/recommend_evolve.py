"""NSGA-II over the surrogates' predictions with no host in the loop: ``BlackBoxMFDGPFitter.recommend(search="evolve")``.

The recommendation of the BO loop is the set of probably-feasible, non-dominated rows of the surrogates' top-fidelity predictive
means (``functional.pareto_mask``).  On a fixed random grid it measures the grid: ``RecommendEvolve`` evolves a population against
the same predictions under the same feasibility rule.  The population logic is util/pareto_evolve.py ``NsgaEngine``
(csrc/pareto_evolve.hip); the values come from a predict group (util/predict_group.py) built for T = Np rows over the fitter's
unconditioned models, objectives first, and mobocmf_recommend_scores (csrc/recommend.hip).  One generation is, in stream order,

    mobocmf_nsga_vary (Np children into rows Np .. 2 Np - 1)  ->  one copy of the children into the group's x
    -> the group's STEP_FORWARD launch  ->  mobocmf_recommend_scores straight into F[:, Np:] and viol[Np:]
    -> mobocmf_nsga_survive on the 2 Np rows, in place, incrementing the generation word

captured once per engine as a HIP graph -- a single chain of nodes -- and replayed.  The group is frozen from the first evaluation
to ``finish()``: a cooperative or frozen-chain group forms its chains once.  Limits: Np even in 4..512, one GPU, one process,
surrogates a predict group takes (M <= 1024); there is no host fallback.
"""
import torch

from .. import _lib
from .. import functional as F
from .. import parallel
from .acq_search import raise_on_info
from .pareto_evolve import NsgaEngine


def choose_group(models, fidelity, T, d):
    """The predict group of ``models`` at T test points: the first of TinyPredictGroup, CoopPredictGroup, PanelPredictGroup and
    SplitPredictGroup (the latter two without gradients) whose ``why_not`` is None for every model -- the speed rule is off,
    there is no layer-path alternative here.  ValueError quoting every class's reason where none fits."""
    from .coop_step import CoopPredictGroup
    from .panel_predict import PanelPredictGroup, SplitPredictGroup
    from .tiny_step import TinyPredictGroup
    reasons = []
    for cls, kw in ((TinyPredictGroup, {}), (CoopPredictGroup, {}), (PanelPredictGroup, dict(want_gradients=False)),
                    (SplitPredictGroup, dict(want_gradients=False))):
        why = [cls.why_not(m, fidelity, T, d) for m in models]
        if all(w is None for w in why):
            return cls(models, fidelity, T, d, **kw)
        reasons.append("%s: model %d: %s" % next((cls.__name__, i, w) for i, w in enumerate(why) if w is not None))
    raise ValueError("RecommendEvolve: no predict group takes these surrogates at T = %d, d = %d (%s)" % (T, d, "; ".join(reasons)))


class RecommendEvolve(NsgaEngine):
    """``NsgaEngine`` over the predictions of ``models`` at layer ``fidelity``: the first ``n_obj`` are the objectives (their
    predictive means, minimised), the rest constraints, feasible when Phi(mbar / sqrt(v)) > ``p_min`` on the noise-free variance
    -- ``functional.pareto_mask``'s rule, graded by mobocmf_recommend_scores.  ``scale`` (len(models), 2): (shift, factor) per
    model.  ``group``: the predict group to evaluate through (built for T = Np on the current stream), default ``choose_group``.

    ``score(X)`` scores any rows through the same group; ``finish()``, after the result is fetched, thaws the group and reports
    what its launches left behind."""

    def __init__(self, models, n_obj, fidelity, Np, d, seed, p_min=0.999, scale=None, options=None, group=None):
        _lib.require_device()
        if parallel.world()[1] != 1:
            raise ValueError("RecommendEvolve: one process only (the surrogates of a process group are sharded over its ranks)")
        models = list(models)
        Np, d, n_obj = int(Np), int(d), int(n_obj)
        if not 1 <= n_obj <= min(len(models), _lib.PARETO_MAX_K) or len(models) > 64:
            raise ValueError("RecommendEvolve: 1..%d objectives among at most 64 models (got %d of %d)"
                             % (_lib.PARETO_MAX_K, n_obj, len(models)))
        if not 0.0 < float(p_min) < 1.0:
            raise ValueError("RecommendEvolve: p_min inside (0, 1) (got %r)" % (p_min,))
        dev = next(models[0].parameters()).device
        self._allocate(Np, d, n_obj, len(models) - n_obj, seed, options, dev)
        self.group = choose_group(models, fidelity, Np, d) if group is None else group
        g = self.group
        if g.T != Np or g.d != d or len(g.models) != len(models) or g.stream is not None:
            raise ValueError("RecommendEvolve: a predict group over the models for T = Np test points on the current stream")
        self.p_min, self.z_min = float(p_min), F.recommend_z_min(p_min)
        self.scale = None if scale is None else torch.as_tensor(scale, dtype=torch.float64).reshape(len(models), 2).to(dev).contiguous()

    # ------------------------------------------------------------------ the launches
    def _scores(self, F_out, ldf, viol_out):
        g, p = self.group, F._ptr
        _lib.check(self.lib.mobocmf_recommend_scores(p(g.moments), self.n_obj, self.n_con, self.Np, g.S, p(self.scale), self.p_min,
                                                     self.z_min, p(F_out), ldf, p(viol_out), F._stream()),
                   "mobocmf_recommend_scores")

    def _evaluate(self, row0):
        Np, g = self.Np, self.group
        g.freeze()
        g.x.copy_(self.X[row0:row0 + Np])
        g._launch(_lib.STEP_FORWARD)
        self._scores(self.F[:, row0:], 2 * Np, None if self.viol is None else self.viol[row0:])

    def score(self, X):
        """(F (n_obj, n), viol (n,)) of the rows ``X`` (n, d), device tensors: chunks of Np rows through the group, the last one
        padded by repeating its last row.  No host read."""
        Np = self.Np
        with torch.no_grad(), torch.cuda.device(self.X.device):
            X = torch.as_tensor(X, dtype=torch.float64).reshape(-1, self.d).to(self.X.device)
            n = X.shape[0]
            if n == 0:
                return self.F.new_zeros(self.n_obj, 0), self.F.new_zeros(0)
            chunks = (n + Np - 1) // Np
            Xp = torch.cat((X, X[-1:].repeat(chunks * Np - n, 1))) if chunks * Np > n else X
            Fg, vg = self.F.new_zeros(self.n_obj, chunks * Np), self.F.new_zeros(chunks * Np)
            self.group.freeze()
            for c in range(chunks):
                self.group.x.copy_(Xp[c * Np:(c + 1) * Np])
                self.group._launch(_lib.STEP_FORWARD)
                self._scores(Fg[:, c * Np:], chunks * Np, vg[c * Np:] if self.n_con else None)
            return Fg[:, :n], vg[:n]

    def info_words(self):
        """The models' Cholesky verdicts (int32 words, 0: fine) as one device tensor, or None; no synchronisation."""
        words = [w.reshape(-1) for w in self.group.info_words]
        return torch.cat(words) if words else None

    def finish(self):
        """Ends the search once its result is fetched: raises on a model's info word (synchronising: one read) and thaws the
        group -- a cooperative group reports an abandoned in-launch wait there."""
        try:
            words = self.info_words()
            if words is not None:
                raise_on_info(words.cpu(), "recommendation search")
        finally:
            self.group.thaw()
