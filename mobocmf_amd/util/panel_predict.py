"""Predictive moments of fitted surrogates with 128 < M <= 1024 inducing points, and their gradient w.r.t. the test points, against
FROZEN chains: mobocmf_frozen_predict (M <= 512) and mobocmf_frozen_predict_split (M <= 1024) (csrc/frozen_predict.hip).

The one-launch predict groups stop at M = 128 (util/tiny_step.py TinyPredictGroup, util/coop_step.py CoopPredictGroup); beyond,
an acquisition search evaluated every iterate through the layer entry points -- five launches per layer forward, as many again
backward, for T S = 125 columns.  ``PanelPredictGroup`` has the surface of those groups that ``DeviceAcqSearch``
(util/acq_search.py) and ``JESMOC_MFDGP`` drive: one launch for the moments of ALL models of a fidelity (MOBOCMF_STEP_FORWARD), one
more for d / dX (MOBOCMF_STEP_INPUT_GRADIENTS).  The M x M chain of every layer is the layer's own (``layer.freeze_chain()``: the
jitter ladder, the host check and NotPSDError all happen there, before any launch of a search).

``SplitPredictGroup`` is the same group on mobocmf_frozen_predict_split: panels of 8 columns, which fit a CU's LDS up to M = 1024,
and the S replicas of a test point split over workgroups, whose partial gradients meet in the group's ``work`` buffer
(DESIGN.md 5.6.2).  ``JESMOC_MFDGP`` uses it where ``PanelPredictGroup`` stops (M > 512).
"""
import ctypes

import torch

from .. import _lib
from . import tiny_step as TS
from .predict_group import PredictGroup

MIN_M = _lib.COOP_MAX_M + 1      # up to COOP_MAX_M the cooperative one-launch group is the engine
MAX_M = _lib.FROZEN_MAX_M
SPLIT_MAX_M = _lib.FROZEN_SPLIT_MAX_M


def why_not(model, fidelity, T, d, on_gpu=True, max_m=MAX_M):
    """None when ``model``'s predictive moments at T test points up to layer ``fidelity`` fit mobocmf_frozen_predict, else the
    reason as a sentence."""
    try:
        layers = model._layers()[:fidelity + 1]
        M = layers[0].variational_strategy._inducing_points.shape[0]
        S = model.num_samples_for_acquisition
    except (AttributeError, IndexError):
        return "not an MFDGP with layer %d" % fidelity
    if len(layers) != fidelity + 1:
        return "the model has no layer %d" % fidelity
    if not MIN_M <= M <= max_m:
        return "M = %d inducing points (this kernel takes %d .. %d)" % (M, MIN_M, max_m)
    if not 1 <= d <= _lib.TINY_MAX_D:
        return "d = %d input columns (at most %d)" % (d, _lib.TINY_MAX_D)
    if fidelity > 0 and not 2 <= S <= _lib.MAX_XDIV:
        return "S = %d samples for acquisition (2 .. %d)" % (S, _lib.MAX_XDIV)
    if T < 1 or T * (S if fidelity > 0 else 1) > _lib.ACQ_MAX_COLUMNS:
        return "T S = %d columns (1 .. %d)" % (T * S, _lib.ACQ_MAX_COLUMNS)
    if any(layer.samples.numel() != S for layer in layers[1:]):
        return "a layer whose fixed samples are not the model's num_samples_for_acquisition"
    if not TS.structure_fits(model, fidelity + 1, d, max_m, training=False, on_gpu=on_gpu):
        return "the structure (tiny_step.structure_fits: <= 3 layers of the expected kinds sharing one Z_x and one jitter, " \
               "softplus / Interval constraints, float64 contiguous parameters%s)" % (" on the GPU" if on_gpu else "")
    return None


def fits_predict(model, fidelity, T, d, on_gpu=True):
    """The gate of ``PanelPredictGroup``, next to tiny_step.fits_predict and coop_step.fits_predict."""
    return why_not(model, fidelity, T, d, on_gpu=on_gpu) is None


def why_not_split(model, fidelity, T, d, on_gpu=True):
    """``why_not`` for mobocmf_frozen_predict_split: the same gate with M in MIN_M .. SPLIT_MAX_M."""
    return why_not(model, fidelity, T, d, on_gpu=on_gpu, max_m=SPLIT_MAX_M)


def fits_predict_split(model, fidelity, T, d, on_gpu=True):
    """The gate of ``SplitPredictGroup``."""
    return why_not_split(model, fidelity, T, d, on_gpu=on_gpu) is None


def describe(rec, chains, samples, S, T, d, x, top_mean, top_var, seed_gmean=None, seed_gvar=None, grad=None, work=None):
    """Fills one mobocmf_frozen_predict_model ``rec`` from the layers' FrozenChain objects (``chains``: their state bytes, Zx, zf
    and packed hyper-parameters) and fixed ``samples`` (per layer; None for layer 0); the other arguments are tensors (or
    None; ``work``: the split entry point's).  Returns the tensors the record points at."""
    L = len(chains)
    rec.L, rec.M, rec.d, rec.S, rec.T = L, chains[0].M, d, (S if L > 1 else 1), T
    keep = []
    for l, fc in enumerate(chains):
        if fc.kind != (1 if l else 0) or fc.M != rec.M or fc.d != d:
            raise _lib.MobocmfError("frozen predict: layer %d is not a kind-%d layer of M = %d, d = %d" % (l, 1 if l else 0, rec.M, d))
        rec.kind[l] = fc.kind
        rec.chain[l], rec.Zx[l], rec.hyp[l] = fc.state.data_ptr(), fc.Zx.data_ptr(), fc.hyp.data_ptr()
        rec.zf[l] = fc.zf.data_ptr() if l else None
        rec.samples[l] = samples[l].data_ptr() if l else None
        keep += [fc.state, fc.Zx, fc.hyp] + ([fc.zf, samples[l]] if l else [])
    for l in range(L, _lib.TINY_MAX_LAYERS):
        rec.kind[l], rec.chain[l], rec.Zx[l], rec.zf[l], rec.hyp[l], rec.samples[l] = 0, None, None, None, None, None
    ptr = lambda t: None if t is None else t.data_ptr()
    rec.x, rec.top_mean, rec.top_var = ptr(x), ptr(top_mean), ptr(top_var)
    rec.seed_gmean, rec.seed_gvar, rec.grad, rec.work = ptr(seed_gmean), ptr(seed_gvar), ptr(grad), ptr(work)
    return keep


class PanelPredictGroup(PredictGroup):
    """Predictive moments of SEVERAL fitted models with 128 < M <= 512 at the same T test points in ONE launch, their gradient
    w.r.t. the test points in one more: a ``PredictGroup`` (util/predict_group.py) as ``TinyPredictGroup`` is one.
    ``want_gradients=False``: a group for values only (the raw candidates of a search) has no seeds and no gx.

    Inside ``freeze()`` ... ``thaw()`` the parameters are constants and the layers' chains are formed once, by ``freeze()``
    (shared with ``MFDGP.frozen_chains()`` where that context is active); a launch outside forms them first."""
    _frozen = False
    _entry = "mobocmf_frozen_predict"

    @classmethod
    def why_not(cls, model, fidelity, T, d, on_gpu=True):
        return why_not(model, fidelity, T, d, on_gpu=on_gpu)

    def __init__(self, models, fidelity, T, d, stream=None, want_gradients=True):
        _lib.require_device()
        self.models = list(models)
        self.device = next(self.models[0].parameters()).device
        self.stream = stream
        self.fidelity, self.T, self.d = fidelity, int(T), int(d)
        n, L = len(self.models), fidelity + 1
        self.S = self.models[0].num_samples_for_acquisition if L > 1 else 1
        for i, model in enumerate(self.models):
            reason = self.why_not(model, fidelity, self.T, self.d)
            if reason is None and L > 1 and model.num_samples_for_acquisition != self.S:
                reason = "S differs from the first model's"
            if reason is not None:
                raise _lib.MobocmfError("%s: model %d does not fit: %s" % (type(self).__name__, i, reason))
        ncol = self.T * self.S
        z = lambda *shape: torch.zeros(*shape, dtype=torch.float64, device=self.device)
        self.x, self.moments = z(self.T, self.d), z(n, 2, ncol)
        self.want_gradients = bool(want_gradients)
        self.seeds, self.gx = (z(n, 2, ncol), z(n, self.T, self.d)) if want_gradients else (None, None)
        self._samples = [[None] + [layer.samples.detach().reshape(-1).to(self.device, torch.float64).contiguous()
                                   for layer in m._layers()[1:L]] for m in self.models]
        self.host = (_lib.FrozenPredictModel * n)()
        self._dev_table = torch.zeros(ctypes.sizeof(self.host), dtype=torch.uint8, device=self.device)
        self._chains, self.info_words = None, []
        self.work = self._allocate_work()

    def _allocate_work(self):
        """(n, doubles) scratch of the entry point, or None: mobocmf_frozen_predict needs none."""
        return None

    # ------------------------------------------------------------------ the chains
    def _form_chains(self):
        """Every layer's chain through ``layer.freeze_chain()`` in eval mode (a model inside ``frozen_chains()`` hands out the
        ones it has), the descriptors pointed at them, the table uploaded.  Synchronising (the layers' host check)."""
        L = self.fidelity + 1
        self._chains, self._keep = [], []
        for i, model in enumerate(self.models):
            model.eval()
            try:
                if model._frozen is not None:
                    chains = model._frozen_chains(L)
                else:
                    chains = [layer.freeze_chain() for layer in model._layers()[:L]]
            finally:
                model.train()
            self._chains.append(chains)
            sd = (None, None) if self.seeds is None else (self.seeds[i, 0], self.seeds[i, 1])
            self._keep += describe(self.host[i], chains, self._samples[i], self.S, self.T, self.d, self.x, self.moments[i, 0],
                                   self.moments[i, 1], sd[0], sd[1], None if self.gx is None else self.gx[i],
                                   None if self.work is None else self.work[i])
        self.info_words = [fc.info for chains in self._chains for fc in chains]
        self._dev_table.copy_(torch.frombuffer(bytearray(bytes(self.host)), dtype=torch.uint8))
        if self.stream is not None:      # (formed and uploaded on the current stream: the launches on self.stream come after)
            self.stream.wait_stream(torch.cuda.current_stream(self.device))

    def freeze(self):
        """The parameters are constants until ``thaw()``: the chains are formed here, once, before any launch of the search."""
        if not self._frozen:
            self._form_chains()
            self._frozen = True

    def thaw(self):
        """Drops the chains: the parameters may change afterwards.  (``info_words`` keep the verdicts of the last chains.)"""
        self._frozen = False
        self._chains = None

    # ------------------------------------------------------------------ the launches
    def _launch(self, mode):
        if mode == _lib.STEP_INPUT_GRADIENTS and not self.want_gradients:
            raise _lib.MobocmfError("%s: built with want_gradients=False" % type(self).__name__)
        if not self._frozen:
            self._form_chains()      # (kept until the next ones replace them: the launch below reads them)
        stream = self.stream if self.stream is not None else torch.cuda.current_stream(self.device)
        _lib.check(getattr(_lib.require_device(), self._entry)(
            ctypes.cast(self.host, ctypes.c_void_p), ctypes.c_void_p(self._dev_table.data_ptr()), len(self.models), int(mode),
            ctypes.c_void_p(stream.cuda_stream)), self._entry)


class SplitPredictGroup(PanelPredictGroup):
    """``PanelPredictGroup`` for 128 < M <= 1024 on mobocmf_frozen_predict_split: the same surface, freeze / thaw and chain
    sharing.  The parts of a test point's replicas leave their partial d / dX in ``work`` (n, ceil(S / 8) T d doubles, allocated
    once per group; None for fidelity 0 and for a group without gradients), summed by the same call."""
    _entry = "mobocmf_frozen_predict_split"

    @classmethod
    def why_not(cls, model, fidelity, T, d, on_gpu=True):
        return why_not_split(model, fidelity, T, d, on_gpu=on_gpu)

    def _allocate_work(self):
        if not self.want_gradients or self.fidelity == 0:
            return None
        rec, nb = _lib.FrozenPredictModel(), ctypes.c_size_t()
        rec.L, rec.M, rec.d, rec.S, rec.T = self.fidelity + 1, MIN_M, self.d, self.S, self.T      # (the bytes do not depend on M)
        _lib.check(_lib.load().mobocmf_frozen_predict_split_work_bytes(ctypes.byref(rec), _lib.STEP_INPUT_GRADIENTS,
                                                                       ctypes.byref(nb)), "mobocmf_frozen_predict_split_work_bytes")
        return torch.zeros(len(self.models), nb.value // 8, dtype=torch.float64, device=self.device)
