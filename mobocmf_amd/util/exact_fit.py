"""Fitting the exact-GP baselines (models/mfgp.py: ``MFGP``, ``MFGP_lin``) on the device: Adam on -log N(y | 0, K) over the raw
parameters of SEVERAL models at once, one captured step replayed per iteration and ONE device-to-host copy at the end
(csrc/exact_fit.hip, include/mobocmf_hip.h: mobocmf_exact_fit_*).

``_ExactMFGP.fit()`` is the host loop: the covariance from torch ops under autograd, the factorisation on the library, autograd
back through the covariance, ``torch.optim.Adam``, and two reads of the device per iteration, model after model.  Here a step is

    covariance (1 launch, all models)  ->  mobocmf_exact_gp_factor per model  ->  prepare (1 launch: L^-T, alpha)  ->
    K^-1 = L^-T L^-1, one triangular MFMA product per model  ->  gradient sums (1 launch)  ->  update (1 launch)

with the loop's bookkeeping -- best iterate, stop on a non-finite loss, restore -- in the update launch, statement for statement.
The step writes the models' own parameter tensors in place through a pointer table (as mobocmf_adam_multi does): ``data_ptr()``,
``requires_grad`` and ``.grad`` are left alone, and the fitted model needs no copy back.
"""
import ctypes

import torch

from .. import _lib
from .. import functional as F
from .. import gp

MAX_N, MAX_MODELS = _lib.EXACT_FIT_MAX_N, _lib.EXACT_FIT_MAX_MODELS

_SLOTS = ("noise", "os_s", "ls_s", "os_n", "ls_n", "rho")      # MOBOCMF_EXACT_FIT_P_*


def _slots(model):
    """[(raw parameter, constraint or None)] of ``model`` in the order of MOBOCMF_EXACT_FIT_P_* (rho: None for MFKernel)."""
    from ..models.mfgp import MFKernel_lin
    cm, lk = model.covar_module, model.likelihood
    ks, kn = cm.cov_funct_signal, cm.cov_funct_noise
    return [(lk.raw_noise, lk.raw_noise_constraint),
            (ks.raw_outputscale, ks.raw_outputscale_constraint), (ks.base_kernel.raw_lengthscale, ks.base_kernel.raw_lengthscale_constraint),
            (kn.raw_outputscale, kn.raw_outputscale_constraint), (kn.base_kernel.raw_lengthscale, kn.base_kernel.raw_lengthscale_constraint),
            (cm.rho if isinstance(cm, MFKernel_lin) else None, None)]


def _constraint(c):
    """(kind, lo, hi) of a constraint object, or None for one the kernels do not know."""
    if c is None:
        return _lib.EXACT_FIT_IDENTITY, 0.0, 0.0
    if type(c) is gp.Positive:
        return _lib.EXACT_FIT_SOFTPLUS, 0.0, 0.0
    if type(c) is gp.GreaterThan:
        return _lib.EXACT_FIT_SOFTPLUS, c.lower_bound, 0.0
    if type(c) is gp.Interval:
        return _lib.EXACT_FIT_SIGMOID, c.lower_bound, c.upper_bound
    return None


def why_not(model, on_gpu=True):
    """None when ``model`` fits the device fit (mobocmf_exact_fit_*), else the reason as a sentence."""
    from ..models.mfgp import MFKernel, MFKernel_lin, _ExactMFGP
    if not isinstance(model, _ExactMFGP) or type(model.covar_module) not in (MFKernel, MFKernel_lin):
        return "not an exact GP with an MFKernel or MFKernel_lin covariance"
    n, d, nl = model.x_train.shape[0], model.input_dim, model.num_fidelities
    if on_gpu and not model.x_train.is_cuda:
        return "the model is not on the GPU"
    if model.x_train.dtype != torch.float64 or any(p.dtype != torch.float64 for p in model.parameters()):
        return "not a float64 model"
    if not 1 <= n <= MAX_N:
        return "n = %d training rows (the device fit takes 1 .. %d)" % (n, MAX_N)
    if not 1 <= d <= _lib.MAX_D:
        return "d = %d input columns (at most %d)" % (d, _lib.MAX_D)
    if not 1 <= nl <= _lib.EXACT_FIT_MAX_LEVELS:
        return "%d fidelity levels (at most %d)" % (nl, _lib.EXACT_FIT_MAX_LEVELS)
    slots = _slots(model)
    want = [1, 1, d, 1, d, nl - 1]
    for name, (p, c), k in zip(_SLOTS, slots, want):
        if p is None:
            continue
        if p.numel() != k or not p.is_contiguous() or (on_gpu and not p.is_cuda):
            return "parameter %s is not a contiguous tensor of %d elements on the GPU" % (name, k)
        if _constraint(c) is None:
            return "parameter %s carries a constraint the device fit does not know (%s)" % (name, type(c).__name__)
    if len(list(model.parameters())) != sum(p is not None for p, _ in slots):
        return "the model has parameters beyond the noise, two outputscales, two lengthscale vectors and rho"
    return None


class ExactFitResult:
    """What a fit reports.  ``names``: the models' keys (a dict's keys, a list's indices) in column order; ``engines[name]``
    "host" or "device"; ``losses`` (num_iters x models, CPU float64): -mll at the parameters each iteration started from, NaN
    from a stop on; per name ``best_loss``, ``best_iteration`` (None: no finite loss was seen), ``stopped_at`` (None, or the
    iteration whose loss was non-finite), ``restored`` (the best iterate was put back) and ``final_loss`` (at the parameters the
    last update left, before any restore; None when the fit had no iteration)."""

    def __init__(self, names, num_iters):
        self.names = list(names)
        self.losses = torch.full((int(num_iters), len(self.names)), float("nan"), dtype=torch.float64)
        self.engines, self.best_loss, self.best_iteration, self.stopped_at, self.restored, self.final_loss = {}, {}, {}, {}, {}, {}

    def _set(self, name, engine, losses, best_loss, best_iteration, stopped_at, restored, final_loss):
        k = self.names.index(name)
        self.losses[:, k] = torch.as_tensor(losses, dtype=torch.float64)
        self.engines[name], self.best_loss[name], self.best_iteration[name] = engine, best_loss, best_iteration
        self.stopped_at[name], self.restored[name], self.final_loss[name] = stopped_at, bool(restored), final_loss


class ExactGPFitStep:
    """One Adam step on the marginal likelihood of SEVERAL exact GPs (a dict or a list of at most 64 ``MFGP`` / ``MFGP_lin`` on
    the GPU), ``num_iters`` the number of iterations its loss record holds.

    ``step()`` issues the launches of an iteration; ``capture()`` records them once -- on ONE stream, the per-model
    factorisations one after the other: no parallel branches -- and ``replay()`` replays that graph: the iteration count lives
    on the device, so a replay IS the next iteration.  ``finish()`` evaluates the likelihood once more and takes the restore
    decision; ``read()`` is the one device-to-host copy (losses, bests, flags, info words) and returns an ``ExactFitResult``.
    ``gradients()``: the last step's d(-mll) / d(raw parameter), per model and parameter name (for tests).

    Torch ops inside the captured step: none -- every launch is the library's."""

    def __init__(self, models, lr, num_iters=200, betas=(0.9, 0.999), eps=1e-8):
        from ..models.mfgp import MFKernel_lin
        lib = _lib.require_device()
        self.names = list(models.keys()) if isinstance(models, dict) else list(range(len(models)))
        self.models = list(models.values()) if isinstance(models, dict) else list(models)
        nm = len(self.models)
        if not 1 <= nm <= MAX_MODELS:
            raise _lib.MobocmfError("ExactGPFitStep: 1 .. %d models" % MAX_MODELS)
        for name, model in zip(self.names, self.models):
            reason = why_not(model)
            if reason is not None:
                raise _lib.MobocmfError("ExactGPFitStep: model %r does not fit: %s" % (name, reason))
        self.lr, self.betas, self.eps, self.cap = float(lr), (float(betas[0]), float(betas[1])), float(eps), max(1, int(num_iters))
        self.device = dev = self.models[0].x_train.device
        cap = self.cap
        # what read() copies: per model [losses (cap) | best loss | final loss | the factorisation's mll] and eight words
        # (MOBOCMF_EXACT_FIT_W_*; word 6 is the factorisation's info word)
        self._vals = torch.zeros(nm, cap + 3, dtype=torch.float64, device=dev)
        self._words = torch.zeros(nm, _lib.EXACT_FIT_WORDS, dtype=torch.int32, device=dev)
        self.host = (_lib.ExactFitModel * nm)()
        self._keep, self._param_names, self._opt, self._factor = [], [], [], []
        sb, cb = ctypes.c_size_t(), ctypes.c_size_t()
        scratch_bytes = 0
        for i, model in enumerate(self.models):
            rec, cm = self.host[i], model.covar_module
            n, d, nl = model.x_train.shape[0], model.input_dim, model.num_fidelities
            with torch.no_grad():
                x = model.x_train[:, :d].contiguous()
                lev = cm.hip_factors(model.x_train)[0].contiguous()
                y = model.y_train.reshape(-1).contiguous()
            rec.n, rec.d, rec.n_levels, rec.cap, rec.reserved = n, d, nl, cap, 0
            rec.kernel = _lib.EXACT_FIT_KERNEL_LIN if isinstance(cm, MFKernel_lin) else _lib.EXACT_FIT_KERNEL_MIN
            rec.x, rec.lev, rec.y = x.data_ptr(), lev.data_ptr(), y.data_ptr()
            slots = _slots(model)
            total = sum(p.numel() for p, _ in slots if p is not None)
            opt = torch.zeros(4, total, dtype=torch.float64, device=dev)      # best | exp_avg | exp_avg_sq | grad
            by_id = {id(p): k for k, p in model.named_parameters()}
            names, off = {}, 0
            for s, (p, c) in enumerate(slots):
                pr = rec.params[s]
                if p is None:
                    pr.raw = pr.best = pr.exp_avg = pr.exp_avg_sq = pr.grad = None
                    pr.numel, pr.kind, pr.lo, pr.hi = 0, _lib.EXACT_FIT_IDENTITY, 0.0, 0.0
                    continue
                k = p.numel()
                pr.raw = p.data_ptr()
                pr.best, pr.exp_avg, pr.exp_avg_sq, pr.grad = (opt[q, off:off + k].data_ptr() for q in range(4))
                pr.numel = k
                pr.kind, pr.lo, pr.hi = _constraint(c)
                names[by_id[id(p)]] = (off, k, tuple(p.shape))
                off += k
            _lib.check(lib.mobocmf_exact_gp_workspace_bytes(n, 1, ctypes.byref(sb), ctypes.byref(cb)), "mobocmf_exact_gp_workspace_bytes")
            scratch_bytes = max(scratch_bytes, cb.value)
            state = torch.zeros(sb.value, dtype=torch.uint8, device=dev)
            npad = (n + 127) // 128 * 128
            sv = state.view(torch.float64)
            rec.Linv, rec.a = sv[npad * npad:].data_ptr(), sv[2 * npad * npad:].data_ptr()      # (functional._exact_state_views)
            rec.mll, rec.info = self._vals[i, cap + 2:].data_ptr(), self._words[i, 6:].data_ptr()
            rec.losses, rec.stats, rec.words = self._vals[i].data_ptr(), self._vals[i, cap:].data_ptr(), self._words[i].data_ptr()
            work = torch.zeros(F.exact_fit_work_bytes(rec, nm) // 8, dtype=torch.float64, device=dev)
            rec.work = work.data_ptr()
            self._keep += [x, lev, y, state, work]
            self._opt.append(opt)
            self._param_names.append(names)
            self._factor.append((n, npad, y, state, sb.value, work))
        self._scratch = torch.zeros(scratch_bytes, dtype=torch.uint8, device=dev)
        self._dev_table = torch.zeros(ctypes.sizeof(self.host), dtype=torch.uint8, device=dev)
        self._dev_table.copy_(torch.frombuffer(bytearray(bytes(self.host)), dtype=torch.uint8))
        self._graph, self._capture_stream, self._warm = None, None, False
        self.reset()

    why_not = staticmethod(why_not)

    # ------------------------------------------------------------------ views of the work areas (tests, tools)
    def _work(self, i):
        n, npad, _, _, _, work = self._factor[i]
        strips = (n + _lib.EXACT_FIT_STRIP - 1) // _lib.EXACT_FIT_STRIP
        o, S = 3 * npad * npad + npad, _lib.EXACT_FIT_SUMS
        return dict(K=work[:npad * npad].view(npad, npad), LiT=work[npad * npad:2 * npad * npad].view(npad, npad),
                    Kinv=work[2 * npad * npad:3 * npad * npad].view(npad, npad), alpha=work[3 * npad * npad:o],
                    slab=work[o:o + strips * S].view(strips, S), sums=work[o + strips * S:o + strips * S + S])

    def covariance(self, i):
        """The padded training covariance of model ``i`` as the last covariance launch left it (npad x npad view)."""
        return self._work(i)["K"]

    def work(self, i):
        """Views of model ``i``'s work area: K, LiT, Kinv (npad x npad), alpha (npad), slab (strips x 83), sums (83)."""
        return self._work(i)

    def mll_word(self, i):
        return self._vals[i, self.cap + 2:self.cap + 3]

    def info_word(self, i):
        return self._words[i, 6:7]

    # ------------------------------------------------------------------ the launches
    def reset(self):
        """A new fit: iteration 0, no best, no stop, zero Adam state, an empty loss record."""
        with torch.no_grad():
            self._vals.fill_(float("nan"))
            self._words.zero_()
            self._words[:, _lib.EXACT_FIT_W_STOPPED_AT] = -1
            self._words[:, _lib.EXACT_FIT_W_BEST_IT] = -1
            for opt in self._opt:
                opt.zero_()

    def launch_covariance(self):
        F.exact_fit_covariance(self.host, self._dev_table)

    def launch_factorisations(self):
        lib, tune, stream = _lib.require_device(), F.current_tuning(), F._stream()
        for rec, (n, npad, y, state, sb, work) in zip(self.host, self._factor):
            _lib.check(lib.mobocmf_exact_gp_factor(n, ctypes.c_void_p(work.data_ptr()), npad, ctypes.c_void_p(y.data_ptr()),
                                                   ctypes.c_void_p(rec.mll), ctypes.c_void_p(rec.info),
                                                   ctypes.c_void_p(state.data_ptr()), sb, ctypes.c_void_p(self._scratch.data_ptr()),
                                                   self._scratch.numel(), ctypes.byref(tune), stream), "mobocmf_exact_gp_factor")

    def launch_inverses(self):
        """L^-T and alpha (one launch), then K^-1 = L^-T (L^-T)^T per model: the triangular MFMA product of
        functional._ExactGPMLL.backward."""
        lib, tune, stream = _lib.require_device(), F.current_tuning(), F._stream()
        F.exact_fit_prepare(self.host, self._dev_table)
        for n, npad, _, _, _, work in self._factor:
            LiT, Kinv = work.data_ptr() + 8 * npad * npad, work.data_ptr() + 16 * npad * npad
            _lib.check(lib.mobocmf_gemm_f64(2, 1, npad, npad, npad, ctypes.c_void_p(LiT), npad, ctypes.c_void_p(LiT), npad,
                                            ctypes.c_void_p(Kinv), npad, 1.0, 0, ctypes.byref(tune), stream), "mobocmf_gemm_f64")

    def launch_gradient(self):
        F.exact_fit_gradient(self.host, self._dev_table)

    def launch_update(self, mode=_lib.EXACT_FIT_STEP):
        F.exact_fit_update(self.host, self._dev_table, mode, self.lr, self.betas, self.eps)

    def evaluate(self):
        """Covariance and factorisation of every model at its current parameters (the loss words; no gradient)."""
        self.launch_covariance()
        self.launch_factorisations()

    def step(self):
        """One iteration, launch by launch (what ``capture()`` records)."""
        with torch.no_grad():
            self.evaluate()
            self.launch_inverses()
            self.launch_gradient()
            self.launch_update(_lib.EXACT_FIT_STEP)
        self._warm = True

    def launches_per_step(self):
        """(launches of this module and the triangular product, calls of mobocmf_exact_gp_factor) in one step."""
        return 4 + len(self.models), len(self.models)

    def capture(self):
        """Records one step.  The capture pass executes nothing; launches that configure themselves at their first call have
        had it before: everything but the update -- which alone changes parameters -- runs once here if no step has."""
        if self._graph is None:
            if not self._warm:
                with torch.no_grad():
                    self.evaluate()
                    self.launch_inverses()
                    self.launch_gradient()
                self._warm = True
            self._capture_stream = torch.cuda.Stream(device=self.device)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=self._capture_stream, capture_error_mode="thread_local"):
                self.step()
            self._graph = g
        return self._graph

    def replay(self):
        self.capture().replay()

    def finish(self):
        """After the last step: the final loss and the restore decision (fit()'s closing statements)."""
        with torch.no_grad():
            self.evaluate()
            self.launch_update(_lib.EXACT_FIT_FINISH)

    def read(self, num_iters=None, result=None):
        """The ONE device-to-host copy; raises InLaunchWaitAbandoned if a factorisation gave up an in-launch wait."""
        from ..acquisition_functions.JESMOC_MFDGP import _read_once      # (the words ride along in the values' copy)
        num_iters = self.cap if num_iters is None else int(num_iters)
        vals, words = _read_once(self._vals, self._words)
        vals, words = vals.view(len(self.models), -1), words.view(len(self.models), -1)
        if bool((words[:, _lib.EXACT_FIT_W_ABANDONED] != 0).any()):
            F.raise_if_abandoned(-1, "exact-GP device fit")
        res = ExactFitResult(self.names, num_iters) if result is None else result
        for i, name in enumerate(self.names):
            w = words[i]
            best_it, stopped = int(w[_lib.EXACT_FIT_W_BEST_IT]), int(w[_lib.EXACT_FIT_W_STOPPED_AT])
            res._set(name, "device", vals[i, :num_iters], float(vals[i, self.cap]) if best_it >= 0 else None,
                     best_it if best_it >= 0 else None, stopped if stopped >= 0 else None, int(w[_lib.EXACT_FIT_W_RESTORED]) != 0,
                     float(vals[i, self.cap + 1]))
        self.iterations = [int(w[_lib.EXACT_FIT_W_IT]) for w in words]
        self.final_info = [int(w[_lib.EXACT_FIT_W_FINAL_INFO]) for w in words]
        return res

    def gradients(self):
        """{model name: {parameter name: d(-mll) / d raw of the last step}} (clones, the parameters' shapes)."""
        out = {}
        for name, opt, names in zip(self.names, self._opt, self._param_names):
            out[name] = {k: opt[3, off:off + cnt].clone().reshape(shape) for k, (off, cnt, shape) in names.items()}
        return out

    def fit(self, num_iters=None, result=None):
        """``num_iters`` iterations from a fresh state: one step issued directly, the captured step replayed for the others,
        the finish sequence, one read."""
        num_iters = self.cap if num_iters is None else int(num_iters)
        if num_iters > self.cap:
            raise _lib.MobocmfError("ExactGPFitStep: built for %d iterations" % self.cap)
        self.reset()
        if num_iters < 1:
            res = ExactFitResult(self.names, 0) if result is None else result
            for name in self.names:
                res._set(name, "device", torch.zeros(0), None, None, None, False, None)
            return res
        self.step()
        if num_iters > 1:
            graph = self.capture()
            for _ in range(num_iters - 1):
                graph.replay()
        self.finish()
        return self.read(num_iters, result)


def _host_fit(model, name, num_iters, lr, result):
    rec = {}
    model._fit_host(num_iters, lr, record=rec)
    losses = rec["losses"] + [float("nan")] * (num_iters - len(rec["losses"]))
    result._set(name, "host", losses, rec["best"], rec["best_iteration"], rec["stopped_at"], rec["restored"], rec["final"])


def fit_exact_gps(models, num_iters=200, lr=0.05):
    """Fits SEVERAL exact GPs (a dict or a list, at most 64): the models ``why_not`` accepts together on the device, the others
    by the host loop one after the other.  Returns an ``ExactFitResult``; ``result.engines[name]`` says which engine a model took."""
    names = list(models.keys()) if isinstance(models, dict) else list(range(len(models)))
    mods = list(models.values()) if isinstance(models, dict) else list(models)
    if not 1 <= len(mods) <= MAX_MODELS:
        raise _lib.MobocmfError("fit_exact_gps: 1 .. %d models" % MAX_MODELS)
    num_iters = int(num_iters)
    result = ExactFitResult(names, num_iters)
    on_device = {k: m for k, m in zip(names, mods) if why_not(m) is None}
    if on_device:
        step = ExactGPFitStep(on_device, lr, num_iters=num_iters)
        step.fit(num_iters, result=result)
    for k, m in zip(names, mods):
        if k not in on_device:
            _host_fit(m, k, num_iters, lr, result)
    return result
