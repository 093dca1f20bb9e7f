"""Predictive moments of fitted exact-GP baselines (models/mfgp.py: ``MFGP``, ``MFGP_lin``) at the same test points, and their
gradient w.r.t. the test points, against a factorisation formed ONCE: mobocmf_exact_predict (csrc/exact_predict.hip).

``_ExactMFGP.predict`` factorises the n x n training covariance at every call (a fresh ``torch.linalg.cholesky`` under autograd,
or mobocmf_exact_gp_factor without a gradient).  ``ExactGPPredictGroup`` has the surface of the predict groups an acquisition
search drives (util/predict_group.py): one launch for the latent moments of ALL its models (MOBOCMF_STEP_FORWARD), one more for
d / dX (MOBOCMF_STEP_INPUT_GRADIENTS); ``freeze()`` factorises every model once (``_hip_factor``: the verdict is checked there,
gp_NotPSD before any launch of a search) and the descriptors point at L^-1 and a = L^-1 y inside the factorisation's own state.
Every model has its own level: ``MESMOC_MFGP`` evaluates the objectives at the searched fidelity and the constraints at the top.
"""
import ctypes

import torch

from .. import _lib
from .. import functional as F
from .predict_group import PredictGroup

MAX_N = _lib.EXACT_PREDICT_MAX_N


def why_not(model, level, T, d, on_gpu=True):
    """None when ``model``'s latent moments at ``level`` at T test points of d columns fit mobocmf_exact_predict, else the
    reason as a sentence."""
    from ..models.mfgp import MFKernel, MFKernel_lin, _ExactMFGP
    if not isinstance(model, _ExactMFGP) or not isinstance(model.covar_module, (MFKernel, MFKernel_lin)):
        return "not an exact GP with an MFKernel or MFKernel_lin covariance"
    n = model.x_train.shape[0]
    if on_gpu and not model.x_train.is_cuda:
        return "the model is not on the GPU"
    if model.x_train.dtype != torch.float64 or any(p.dtype != torch.float64 for p in model.parameters()):
        return "not a float64 model"
    if not 1 <= n <= MAX_N:
        return "n = %d training rows (this kernel takes 1 .. %d)" % (n, MAX_N)
    if model.input_dim != d or not 1 <= d <= _lib.MAX_D:
        return "d = %d input columns (the model has %d; at most %d)" % (d, model.input_dim, _lib.MAX_D)
    if not 1 <= model.num_fidelities <= _lib.EXACT_PREDICT_MAX_LEVELS or not 0 <= level < model.num_fidelities:
        return "level %d of %d fidelity levels (at most %d)" % (level, model.num_fidelities, _lib.EXACT_PREDICT_MAX_LEVELS)
    if not 1 <= T <= _lib.TOPK_MAX_N:
        return "T = %d test points (1 .. %d)" % (T, _lib.TOPK_MAX_N)
    return None


class ExactGPPredictGroup(PredictGroup):
    """Latent moments of SEVERAL fitted exact GPs, model i at level ``levels[i]``, at the same T test points in ONE launch, their
    gradient w.r.t. the test points in one more: a ``PredictGroup`` with S = 1 (a column is a test point, as for a fidelity-0
    group).  ``want_gradients=False``: a group for values only (the raw candidates of a search) has no seeds and no gx.

    Inside ``freeze()`` ... ``thaw()`` the parameters are constants and every model is factorised once, by ``freeze()``; a
    launch outside factorises first.  ``info_words`` are the factorisations' verdicts (already checked by ``freeze()``)."""
    S = 1
    fidelity = 0      # (what PredictGroup.acquisition_moments asks: no replicas)
    _frozen = False

    @classmethod
    def why_not(cls, model, level, T, d, on_gpu=True):
        return why_not(model, level, T, d, on_gpu=on_gpu)

    def __init__(self, models, levels, T, d, stream=None, want_gradients=True):
        _lib.require_device()
        self.models, self.levels = list(models), [int(l) for l in levels]
        if len(self.models) != len(self.levels) or not 1 <= len(self.models) <= 2 * _lib.ACQ_MAX_PAIRS:
            raise _lib.MobocmfError("ExactGPPredictGroup: one level per model, 1 .. %d models" % (2 * _lib.ACQ_MAX_PAIRS))
        self.device = self.models[0].x_train.device
        self.stream = stream
        self.T, self.d = int(T), int(d)
        for i, (model, level) in enumerate(zip(self.models, self.levels)):
            reason = self.why_not(model, level, self.T, self.d)
            if reason is not None:
                raise _lib.MobocmfError("ExactGPPredictGroup: model %d does not fit: %s" % (i, reason))
        n = len(self.models)
        z = lambda *shape: torch.zeros(*shape, dtype=torch.float64, device=self.device)
        self.x, self.moments = z(self.T, self.d), z(n, 2, self.T)
        self.want_gradients = bool(want_gradients)
        self.seeds, self.gx = (z(n, 2, self.T), z(n, self.T, self.d)) if want_gradients else (None, None)
        self.host = (_lib.ExactPredictModel * n)()
        self._dev_table = torch.zeros(ctypes.sizeof(self.host), dtype=torch.uint8, device=self.device)
        self._keep, self.info_words = None, []

    # ------------------------------------------------------------------ the factorisations
    def _describe(self, rec, i, model, level):
        """Factorises ``model`` and fills its record; returns the tensors the record points at."""
        cm, d, nl = model.covar_module, self.d, model.num_fidelities
        st = model._hip_factor()      # (synchronising: raises gp_NotPSD / InLaunchWaitAbandoned here, before any launch)
        _, Li, a, npad = F._exact_state_views(st)
        with torch.no_grad():
            xtr = model.x_train[:, :d].contiguous()
            lev, _ = cm.hip_factors(model.x_train)
            rows = torch.zeros(nl, model.x_train.shape[1], dtype=torch.float64, device=self.device)
            rows[:, d] = torch.arange(nl, dtype=torch.float64, device=self.device)
            _, sig = cm.hip_factors(rows)      # the kernel's own signal factor of a row at every level (None: all ones)
            sig = torch.ones(nl, dtype=torch.float64, device=self.device) if sig is None else sig.to(torch.float64).contiguous()
            ntab = cm.hip_noise_table(nl, self.device).to(torch.float64).contiguous()
            hyp = [torch.cat([k.outputscale.reshape(1), k.base_kernel.lengthscale.reshape(-1)]).detach().to(torch.float64).contiguous()
                   for k in (cm.cov_funct_signal, cm.cov_funct_noise)]
            kss = float(sig[level] * sig[level] * hyp[0][0] + ntab[level] * hyp[1][0])
        lev = lev.contiguous()
        rec.n, rec.d, rec.T, rec.n_levels, rec.level, rec.reserved, rec.ld = st.n, d, self.T, nl, level, 0, npad
        rec.xtr, rec.lev, rec.sig, rec.ntab = xtr.data_ptr(), lev.data_ptr(), sig.data_ptr(), ntab.data_ptr()
        rec.hyp_s, rec.hyp_n, rec.Linv, rec.a, rec.kss = hyp[0].data_ptr(), hyp[1].data_ptr(), Li.data_ptr(), a.data_ptr(), kss
        rec.x, rec.top_mean, rec.top_var = self.x.data_ptr(), self.moments[i, 0].data_ptr(), self.moments[i, 1].data_ptr()
        if self.want_gradients:
            rec.seed_gmean, rec.seed_gvar = self.seeds[i, 0].data_ptr(), self.seeds[i, 1].data_ptr()
            rec.grad = self.gx[i].data_ptr()
        else:
            rec.seed_gmean, rec.seed_gvar, rec.grad = None, None, None
        rec.work = None      # (mobocmf_exact_predict_work_bytes is 0 for both modes)
        self.info_words.append(st.info.reshape(1))
        return [st, xtr, lev, sig, ntab] + hyp

    def _factorise(self):
        self._keep, self.info_words = [], []
        for i, (model, level) in enumerate(zip(self.models, self.levels)):
            self._keep += self._describe(self.host[i], i, model, level)
        ns = [rec.n for rec in self.host]
        if self.__dict__.setdefault("_ns", ns) != ns:      # (a captured launch carries the grid and the LDS bytes of these)
            raise _lib.MobocmfError("ExactGPPredictGroup: the models' training rows changed (%s -> %s): build a new group"
                                    % (self._ns, ns))
        self._dev_table.copy_(torch.frombuffer(bytearray(bytes(self.host)), dtype=torch.uint8))
        if self.stream is not None:      # (formed and uploaded on the current stream: the launches on self.stream come after)
            self.stream.wait_stream(torch.cuda.current_stream(self.device))

    def freeze(self):
        """The parameters are constants until ``thaw()``: every model is factorised here, once."""
        if not self._frozen:
            self._factorise()
            self._frozen = True

    def thaw(self):
        """Drops the factorisations: the parameters may change afterwards.  (``info_words`` keep the last verdicts.)"""
        self._frozen = False
        self._keep = None

    def noise(self, refresh=False):
        """(n_models,) likelihood noise of the models (constrained values), formed once; ``refresh=True`` re-reads them."""
        if refresh or self._noise is None:
            with torch.no_grad():
                self._noise = torch.stack([m.likelihood.noise.reshape(()) for m in self.models]).to(torch.float64)
        return self._noise

    # ------------------------------------------------------------------ the launches
    def _launch(self, mode):
        if mode == _lib.STEP_INPUT_GRADIENTS and not self.want_gradients:
            raise _lib.MobocmfError("ExactGPPredictGroup: built with want_gradients=False")
        if not self._frozen:
            self._factorise()      # (kept until the next ones replace them: the launch below reads them)
        stream = self.stream if self.stream is not None else torch.cuda.current_stream(self.device)
        F.exact_predict_launch(self.host, self._dev_table, mode, stream=stream)
