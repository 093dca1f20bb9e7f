"""The ELBO step of SMALL surrogates (zero_grad + MFDGP.forward + VariationalELBOMF + backward + Adam,
blackbox_mfdgp_fitter.py:161-171) as ONE launch for a whole group of models: mobocmf_tiny_elbo_step.

At the reference's own sizes -- M = N = tens of points (examples/example_acquisition_mfdgp_forrester/...py:51-62) -- a step
through the layer entry points is ~50 dependent launches of ~4.7 us whatever they compute; here one workgroup per surrogate
runs the whole step as barrier-separated phases (csrc/tiny_step.hip).  ``TinyELBOStep`` has the surface of
``GraphedELBOStep`` that the fitter's training loop uses (step / check / snapshot / loss), for several models at once.
"""
import ctypes
import os

import torch

from .. import _lib
from .. import functional as F
from .. import gp
from .predict_group import PredictGroup

LAYER_PATH_US = 240.0   # what a step of a small surrogate costs through the layer entry points (HIP-graph replay, MI355X)


def estimated_us(M, columns):
    """Duration of one launch, from tools/tiny_sweep.py on MI355X (profiles/r04_tiny_step.txt): a fixed part that grows with
    the chain (M^2) and a part per panel column -- one workgroup does everything, so beyond a few dozen columns at M = 32
    (a few hundred at M = 16) the grid-filling kernels of the layer path win and ``eligible`` says no."""
    return 20.0 + 0.15 * M * M + (M * M / 900.0) * float(sum(columns))


class Kernel:
    """The kernel a step object or a predict group drives: its limits, its entry points, the words of its in-launch waits and
    its launch.  ``max_columns`` / ``max_predict_columns``: rows[l] * S per layer this binding accepts for training / for
    prediction; ``max_coupled_models``: models of one MOBOCMF_STEP_COUPLED launch (None: what the device keeps resident)."""

    def __init__(self, entry, work_bytes_fn, max_m, max_columns, max_predict_columns, max_coupled_models, cooperative):
        self.entry, self.work_bytes_fn = entry, work_bytes_fn
        self.max_m, self.max_columns, self.max_predict_columns = max_m, max_columns, max_predict_columns
        self.max_coupled_models, self.cooperative = max_coupled_models, cooperative

    def sync_words(self, n, coupled):
        """(int64 words, index of the status word) of the in-launch waits of a group of n models; None: the launches wait
        for nothing."""
        if self.cooperative:      # per model 16 words (its arrival counter first), then the grid's counter and the status word
            return 16 * (n + 1), 16 * n + 1
        return (2, 1) if coupled else None      # the coupling record's arrival counter and its status word

    def launch(self, group, mode, lr, beta1, beta2, eps):
        """Enqueues one launch over ``group``'s descriptor table on its stream (None: the current one).  The cooperative kernel
        runs ``group.wgs_per_model`` workgroups per model (0: chosen by the library from the widest phase) and leaves what it
        ran with in ``group.wgs_used``."""
        fn = getattr(_lib.require_device(), self.entry)
        host, table = ctypes.cast(group.host, ctypes.c_void_p), ctypes.c_void_p(group._dev_table.data_ptr())
        stream = group.stream if group.stream is not None else torch.cuda.current_stream(group.device)
        stream = ctypes.c_void_p(stream.cuda_stream)
        if not self.cooperative:
            _lib.check(fn(host, table, len(group.models), lr, beta1, beta2, eps, int(mode), stream), self.entry)
            return
        used = ctypes.c_int32(0)
        _lib.check(fn(host, table, len(group.models), int(group.wgs_per_model), ctypes.c_void_p(group.in_launch_sync().ptr(0)),
                      lr, beta1, beta2, eps, int(mode), ctypes.byref(used), stream), self.entry)
        group.wgs_used = used.value


# one workgroup per surrogate (csrc/tiny_step.hip)
TINY = Kernel("mobocmf_tiny_elbo_step", "mobocmf_tiny_work_bytes", _lib.TINY_MAX_M, 1024, 4096, 64, cooperative=False)


def _hyper_params(layer):
    return [getattr(m, n) for m, n in gp._hyper_sources(layer.covar_module, layer.kind)]


def _likelihood(model, l):
    return getattr(model, model.name_hidden_layer_likelihood + str(l))


def rows_per_layer(fidelities, L):
    """Layer l runs on the rows of fidelity >= l."""
    fidv = fidelities.reshape(-1)
    return [int((fidv >= l).sum()) for l in range(L)]


def structure_fits(model, L, d, max_m, training, on_gpu=True):
    """The structural limits both kernels share, for the first ``L`` layers of ``model`` (None: all) on d input columns: <= 3 of the
    expected kinds sharing one jitter and one set of <= ``max_m`` inducing inputs (Z~_l = [Z_x, m_{l-1}]), d <= 8, softplus /
    Interval constraints, float64 contiguous parameters (``on_gpu``: on the GPU); ``training``: model and layers in training
    mode (prediction runs the eval branch whatever the flags say)."""
    try:
        layers = model._layers() if L is None else model._layers()[:L]
        if not (1 <= len(layers) <= _lib.TINY_MAX_LAYERS) or model.use_only_highest_fidelity or not (1 <= d <= _lib.TINY_MAX_D):
            return False
        if training and model._eval_mode:
            return False
        Z0 = layers[0].variational_strategy._inducing_points
        M = Z0.shape[0]
        if not (1 <= M <= max_m) or Z0.shape[1] != d or (on_gpu and not Z0.is_cuda):
            return False
        jit = layers[0].variational_strategy.jitter_val
        for l, layer in enumerate(layers):
            vs = layer.variational_strategy
            vd = vs._variational_distribution
            Zl = vs._inducing_points
            if layer.kind != (0 if l == 0 else 1) or vs.jitter_val != jit or Zl.shape[0] != M or (training and not layer.training):
                return False
            if l and vs.Zx is not Z0 and not torch.equal(Zl[:, :-1], Z0):      # layers >= 1 share Z_x; their f column is m_{l-1} (F9)
                return False
            lik = _likelihood(model, l)
            c = lik.raw_noise_constraint
            if type(c) is not gp.Interval or not (c.upper_bound > c.lower_bound) or c.upper_bound == float("inf"):
                return False
            ps = _hyper_params(layer) + [vd.variational_mean, vd.chol_variational_covar, lik.raw_noise]
            if not all((p.is_cuda or not on_gpu) and p.dtype == torch.float64 and p.is_contiguous() for p in ps):
                return False
            if not all(type(getattr(m, n + "_constraint")) is gp.Positive
                       for m, n in gp._hyper_sources(layer.covar_module, layer.kind)):
                return False
        return True
    except AttributeError:
        return False


def fits_predict(model, fidelity, T, d, speed_rule=True, kernel=TINY, on_gpu=True):
    """True when ``model``'s predictive moments at T test points up to layer ``fidelity`` fit the one-launch kernel
    (``structure_fits``; the training flags do not matter), every layer has the model's number of fixed samples and the
    columns are within the kernel's limit -- and, with ``speed_rule``, few enough for one workgroup to beat the layer path."""
    try:
        if not structure_fits(model, fidelity + 1, d, kernel.max_m, training=False, on_gpu=on_gpu):
            return False
        layers = model._layers()[:fidelity + 1]
        S = model.num_samples_for_acquisition
        cols = [T] + [T * S] * (len(layers) - 1)
        if max(cols) > kernel.max_predict_columns or any(layer.samples.numel() != S for layer in layers[1:]):
            return False
        M = layers[0].variational_strategy._inducing_points.shape[0]
        return not (speed_rule and estimated_us(M, cols) > LAYER_PATH_US)
    except AttributeError:
        return False


def eligible(model, x, fidelities, speed_rule=True, kernel=TINY):
    """True when ``model`` on the batch ``x`` fits the one-launch step of ``kernel``: ``structure_fits`` in training mode, fixed
    inducing inputs, float64 data on the GPU, rows[l] * S within the kernel's limit, every fidelity's prefix non-empty -- and,
    with ``speed_rule``, small enough for one workgroup to beat the layer path (estimated_us)."""
    try:
        if not x.is_cuda or x.dtype != torch.float64 or x.dim() != 2:
            return False
        if not structure_fits(model, None, x.shape[1], kernel.max_m, training=True):
            return False
        layers = model._layers()
        if any(layer.variational_strategy._inducing_points.requires_grad for layer in layers):
            return False
        S = model.num_samples_for_training
        N = fidelities.numel()
        if N != x.shape[0] or N * max(S, 1) > kernel.max_columns:
            return False
        counts = rows_per_layer(fidelities, len(layers))
        if counts[0] != N or counts[-1] < 1:
            return False
        M = layers[0].variational_strategy._inducing_points.shape[0]
        return not (speed_rule and estimated_us(M, [c * (S if l else 1) for l, c in enumerate(counts)]) > LAYER_PATH_US)
    except AttributeError:
        return False


class Descriptor:
    """Fills one mobocmf_tiny_model record ``rec`` for the first ``L`` layers of ``model``: the header, per layer the raw
    parameters, m, L_S, the noise parameter with its bounds, Z_x, the jitter and the eps / rng pointers.  ``segments``: the flat
    vector of grad / adam_m / adam_v as [(parameter, offset, length)], checked against mobocmf_tiny_flat_len.  Everything up to
    ``allocate`` runs on whatever device the model is on (the library's size queries are host code)."""

    def __init__(self, rec, model, L, d, S, rows, kl_scale, eps=None, natgrad=False, branch=0):
        """``rows[l]``: the rows of layer l; ``eps[l]``: given draws of layer l >= 1 (None: the layer's rng stream);
        ``natgrad``: q(u) of every layer whose m AND L_S both require a gradient is moved by the natural-gradient launch --
        ``natural`` lists them as (layer, M, flat offset of m, of L_S) and their trainable bits 7 and 8 are cleared."""
        self.rec, self.model, self.layers = rec, model, model._layers()[:L]
        self.keep, self.segments, self.natural, self.eps = [], [], [], [None] * L
        Z0 = self.layers[0].variational_strategy._inducing_points
        rec.L, rec.M, rec.d, rec.S, rec.N = L, Z0.shape[0], d, S, rows[0]
        rec.branch, rec.kl_scale, rec.jitter = branch, kl_scale, self.layers[0].variational_strategy.jitter_val
        Zx = Z0.detach().contiguous()
        rec.Zx = Zx.data_ptr()
        self.keep.append(Zx)
        off = 0
        for l, layer in enumerate(self.layers):
            vd = layer.variational_strategy._variational_distribution
            lik = _likelihood(model, l)
            rec.rows[l] = rows[l]
            tr = 0
            for s, p in enumerate(_hyper_params(layer)):
                rec.raw[l][s] = p.data_ptr()
                tr |= int(p.requires_grad) << s
                self.segments.append((p, off, p.numel()))
                off += p.numel()
            natural = natgrad and vd.variational_mean.requires_grad and vd.chol_variational_covar.requires_grad
            if natural:
                Ml = vd.variational_mean.numel()
                self.natural.append((l, Ml, off, off + Ml))
            for bit, p in ((7, vd.variational_mean), (8, vd.chol_variational_covar)):
                tr |= int(p.requires_grad and not natural) << bit
                self.segments.append((p, off, p.numel()))
                off += p.numel()
            rec.m[l], rec.L_S[l] = vd.variational_mean.data_ptr(), vd.chol_variational_covar.data_ptr()
            # (the eval branch never updates: its record keeps the bits 0)
            rec.trainable[l] = 0 if branch else tr | int(lik.raw_noise.requires_grad) << 9
            rec.raw_noise[l] = lik.raw_noise.data_ptr()
            rec.noise_lo[l], rec.noise_hi[l] = lik.raw_noise_constraint.lower_bound, lik.raw_noise_constraint.upper_bound
            if l and eps is not None and eps[l] is not None:
                self.set_eps(l, eps[l])
            elif l:
                rng = layer._rng(Zx.device)
                rec.rng[l] = rng.data_ptr()
                self.keep.append(rng)
        for l in range(L):
            self.segments.append((_likelihood(model, l).raw_noise, off + l, 1))
        self.flat_len = off + L
        flat = ctypes.c_int64()
        _lib.check(_lib.load().mobocmf_tiny_flat_len(ctypes.byref(rec), ctypes.byref(flat)), "mobocmf_tiny_flat_len")
        assert flat.value == self.flat_len, (flat.value, self.flat_len)

    def set_eps(self, l, e):
        self.eps[l] = e
        self.rec.eps[l] = e.data_ptr()
        self.keep.append(e)

    @classmethod
    def for_training(cls, rec, model, d, fidelities, num_data, natgrad=False):
        """The full-batch ELBO step on rows ordered by descending fidelity: kl_scale = N / num_data."""
        L = len(model._layers())
        rows = rows_per_layer(fidelities, L)
        return cls(rec, model, L, d, model.num_samples_for_training, rows, rows[0] / float(num_data), natgrad=natgrad)

    @classmethod
    def for_prediction(cls, rec, model, fidelity, n_test, d):
        """The eval branch at ``n_test`` points up to layer ``fidelity``: eval_mode's draws are the layers' fixed samples, tiled
        over the test points (mfdgp_hidden_layer.py:263-270); no row is scored."""
        L = fidelity + 1
        eps = [None] + [layer.samples.reshape(-1).to(torch.float64).repeat(n_test).contiguous() for layer in model._layers()[1:L]]
        return cls(rec, model, L, d, model.num_samples_for_acquisition if L > 1 else 1, [n_test] * L, 0.0, eps=eps, branch=1)

    def allocate(self, kernel, dev):
        """Sizes and allocates the workspace of ``kernel`` for this record.  MOBOCMF_POISON (as functional._scratch): NaN-filled,
        so a read of anything the launch did not write shows."""
        wb = ctypes.c_size_t()
        _lib.check(getattr(_lib.load(), kernel.work_bytes_fn)(ctypes.byref(self.rec), ctypes.byref(wb)), kernel.work_bytes_fn)
        work = torch.full((wb.value // 8,), float("nan") if os.environ.get("MOBOCMF_POISON") else 0.0,
                          dtype=torch.float64, device=dev)
        self.rec.work = work.data_ptr()
        return work


class _OneLaunchGroup:
    """What the step objects and the predict groups share: the descriptor table of their models in host and device memory,
    the tensors it points at, the words of the in-launch waits and the launch of ``kernel``."""
    kernel = TINY
    coupled = False        # the launches meet at the barrier of a coupling record (the conditioned step)
    stream = None          # the launches' stream; None: the current one
    wgs_per_model = 0      # the cooperative kernel's workgroups per model; 0: chosen by the library from the widest phase

    def _new_table(self, models, dev):
        self.models, self.device = list(models), dev
        self.host = (_lib.TinyModel * len(self.models))()
        self._keep = []          # tensors the descriptors point at

    def _upload(self):
        """The table as the kernels read it.  It and everything it points at was allocated, zero-filled and uploaded on the
        CURRENT stream: the launches on ``self.stream`` come after."""
        self._dev_table = torch.frombuffer(bytearray(bytes(self.host)), dtype=torch.uint8).to(self.device)
        self._order_after_setup()

    def _order_after_setup(self):
        """Without this edge a fill kernel could still be pending when the first launch starts (found with a cooperative launch
        whose arrival counters were zeroed under it: tools/coop_concurrency_probe.py)."""
        if self.stream is not None:
            self.stream.wait_stream(torch.cuda.current_stream(self.device))

    def in_launch_sync(self):
        """The counters and status word of the launches' in-launch waits (functional.InLaunchSync), made on first use; None
        for a kernel without such waits."""
        sync = self.__dict__.get("sync")
        if sync is None:
            sync = self.sync = self._new_sync()
            if sync is not None:
                self._order_after_setup()      # (zero-filled on the current stream)
        return sync

    def _new_sync(self):
        layout = self.kernel.sync_words(len(self.models), self.coupled)
        if layout is None:
            return None
        return F.InLaunchSync(torch.zeros(layout[0], dtype=torch.int64, device=self.device), layout[1], self.stream)

    def _launch(self, mode):
        """mode: _lib.STEP_* (do_update of mobocmf_tiny_elbo_step / mobocmf_coop_elbo_step); no update in the forward-only and
        input-gradient modes, so Adam's settings do not matter here."""
        self.kernel.launch(self, mode, 0.0, 0.9, 0.999, 1e-8)


class TinyELBOStep(_OneLaunchGroup):
    """``step()`` == one full-batch ELBO step of EVERY model of the group, one launch.  ``models[i]`` trains on
    ``(xs[i], ys[i], fids[i])`` (y: (N, 1) or (N,); fidelities as the ELBO takes them).  The rows are ordered once by
    descending fidelity (``row_order[i]``; a full-batch ELBO is a sum over rows) and layer l runs on the rows of fidelity
    >= l, as ``GraphedELBOStep(prune_rows=True)``.  ``losses`` is an (n, 3) device tensor: ELBO, scaled KL, -ELBO per model,
    as of the last step (before its update)."""

    def __init__(self, models, num_data, xs, ys, fids, lr, betas=(0.9, 0.999), eps=1e-8, stream=None, fixed_eps=None,
                 want_grad=False, prepared=None, force=False, variational_optimizer="adam", natgrad_gamma=0.1,
                 natgrad_gamma_init=1e-4, natgrad_warmup_steps=100):
        """``force``: take every size the kernel accepts, also those where the layer path is faster (tests, sweeps).
        ``variational_optimizer="natgrad"``: q(u) of every layer whose ``variational_mean`` AND ``chol_variational_covar`` both
        require a gradient moves by natural gradients (schedule ``natgrad_gamma`` / ``natgrad_gamma_init`` /
        ``natgrad_warmup_steps`` as ``GraphedELBOStep``): the one-launch step leaves those two tensors alone (trainable bits
        7 and 8 cleared) and writes its flat gradient, a second launch (mobocmf_natgrad_small_step, one workgroup per layer)
        moves them; Adam keeps every other parameter, and a layer with either tensor frozen keeps today's path.
        ``prepared`` (TinyConditionedStep): per model a dict with the rows ALREADY in the kernel's order and the optional
        fields of mobocmf_tiny_model -- x, y, fid, rows, row_weight, kl_scale, seeds (bool), rand (row0, rows), xrng, eps
        (per layer, prefix columns)."""
        _lib.require_device()
        if variational_optimizer not in ("adam", "natgrad"):
            raise ValueError("variational_optimizer must be 'adam' or 'natgrad' (got %r)" % (variational_optimizer,))
        self.variational_optimizer = variational_optimizer
        self.natgrad_gamma, self.natgrad_gamma_init = float(natgrad_gamma), float(natgrad_gamma_init)
        self.natgrad_warmup_steps = int(natgrad_warmup_steps)
        if variational_optimizer == "natgrad" and not (0.0 < self.natgrad_gamma_init <= self.natgrad_gamma
                                                       and self.natgrad_warmup_steps >= 0):
            raise ValueError("%s: 0 < natgrad_gamma_init <= natgrad_gamma and natgrad_warmup_steps >= 0" % type(self).__name__)
        dev = (xs[0] if prepared is None else prepared[0]["x"]).device
        self._new_table(models, dev)
        n = len(self.models)
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.stream = stream if stream is not None else torch.cuda.Stream(device=dev)
        self.losses = torch.zeros(n, 3, dtype=torch.float64, device=dev)
        self.infos = torch.zeros(n, _lib.TINY_MAX_LAYERS, dtype=torch.int32, device=dev)
        self.steps_done = torch.zeros(n, dtype=torch.int64, device=dev)
        self.row_order, self.layer_rows = [], []
        self.exp_avg, self.exp_avg_sq, self.grads, self._work = [], [], [], []
        self._segments = []      # per model: [(parameter tensor, flat offset, length)]
        self._gflat = {}         # model -> the flat gradient its launches write (want_grad, or a natural-gradient layer)
        self._natural = []       # layers moved by natural gradients: (model, layer, word, M, flat offset of m, of L_S, scale)
        self.num_layers = 0      # layers of all models: one word each in natgrad_steps / skipped / natgrad_info
        self.top_moments, self.seeds, self.x_rows = [], [], []      # prepared models: (2, ncol_top) tensors, the x array
        natgrad = variational_optimizer == "natgrad"
        for i, model in enumerate(self.models):
            prep = None if prepared is None else prepared[i]
            x, y, fid = (xs[i], ys[i], fids[i]) if prep is None else (prep["x"], prep["y"], prep["fid"])
            if not eligible(model, x, fid, speed_rule=not force and not self.kernel.cooperative, kernel=self.kernel):
                raise _lib.MobocmfError("%s: model %d does not fit the one-launch step (see eligible())" % (type(self).__name__, i))
            L, S = len(model._layers()), model.num_samples_for_training
            fidv = fid.reshape(-1).to(torch.float64)
            N = fidv.numel()
            T = self.host[i]
            if prep is None:
                desc = Descriptor.for_training(T, model, x.shape[1], fidv, num_data[i], natgrad)
                order = torch.argsort(fidv, descending=True, stable=True)
                xo, yo, fo = x[order].contiguous(), y.reshape(-1)[order].to(torch.float64).contiguous(), fidv[order].contiguous()
                given = None if fixed_eps is None else fixed_eps[i]
            else:
                desc = Descriptor(T, model, L, x.shape[1], S, [int(r) for r in prep["rows"]], float(prep["kl_scale"]),
                                  natgrad=natgrad)
                order = None
                xo, yo, fo = x.contiguous(), y.reshape(-1).to(torch.float64).contiguous(), fidv.contiguous()
                given = prep.get("eps")
            counts = list(T.rows[:L])
            self.row_order.append(order)
            self.layer_rows.append(counts)
            T.x, T.y, T.fid = xo.data_ptr(), yo.data_ptr(), fo.data_ptr()
            self._keep += [xo, yo, fo]
            for l in range(1, L):
                e = None if given is None else given[l]
                if e is not None and order is not None:      # given for the batch as passed in (N * S values): follow the rows
                    e = e.reshape(N, S)[order]
                if e is not None:
                    desc.set_eps(l, e.reshape(-1)[:counts[l] * S].contiguous())
            if prep is not None:
                ntop = counts[-1] * (S if L > 1 else 1)
                if prep.get("row_weight") is not None:
                    w = prep["row_weight"].to(torch.float64).contiguous()
                    T.row_weight = w.data_ptr()
                    self._keep.append(w)
                tm = torch.zeros(2, ntop, dtype=torch.float64, device=dev)
                T.top_mean, T.top_var = tm[0].data_ptr(), tm[1].data_ptr()
                self.top_moments.append(tm)
                if prep.get("seeds"):
                    sd = torch.zeros(2, ntop, dtype=torch.float64, device=dev)
                    T.seed_gmean, T.seed_gvar, T.seed_scale = sd[0].data_ptr(), sd[1].data_ptr(), float(prep.get("seed_scale", 1.0))
                    self.seeds.append(sd)
                if prep.get("xrng") is not None:
                    T.xrng = prep["xrng"].data_ptr()
                    T.rand_row0, T.rand_rows = prep["rand"]
                    self._keep.append(prep["xrng"])
                self.x_rows.append(xo)
            # (scale: what turns the launch's loss into -ELBO -- the inverse of kl_scale)
            scale = 1.0 if prep is not None else float(num_data[i]) / N
            self._natural += [(i, l, self.num_layers + l, Ml, om, oL, scale) for l, Ml, om, oL in desc.natural]
            self.num_layers += L
            self._keep += desc.keep
            self._segments.append(desc.segments)
            self._work.append(desc.allocate(self.kernel, dev))
            ea, eq = (torch.zeros(desc.flat_len, dtype=torch.float64, device=dev) for _ in range(2))
            self.exp_avg.append(ea)
            self.exp_avg_sq.append(eq)
            T.adam_m, T.adam_v = ea.data_ptr(), eq.data_ptr()
            T.steps_done = self.steps_done[i:i + 1].data_ptr()
            T.out = self.losses[i].data_ptr()
            T.info = self.infos[i].data_ptr()
            if want_grad or desc.natural:
                gflat = torch.zeros(desc.flat_len, dtype=torch.float64, device=dev)
                if want_grad:
                    self.grads.append(gflat)
                self._gflat[i] = gflat
                T.grad = gflat.data_ptr()
        self._snap = None
        self._setup_natgrad()
        self._upload()

    def _setup_natgrad(self):
        """The records of the second launch (functional.NatGradSmallLayers): every natural-gradient layer's m / L_S, their
        segments of the model's flat gradient, its own schedule counter, and as guard the producing launch's info words, its
        in-launch status word (where the kernel has one) and its loss."""
        dev = self.device
        self.skipped = [0] * self.num_layers      # per layer, as of the last check()
        self._natgrad_table = self.natgrad_steps = self.natgrad_words = self.natgrad_skipped = self.natgrad_info = None
        if not self._natural:      # (the default path allocates nothing for this)
            return
        self.natgrad_steps = torch.zeros(self.num_layers, dtype=torch.int64, device=dev)
        self.natgrad_words = torch.zeros(2, self.num_layers, dtype=torch.int32, device=dev)      # one host copy reads both rows
        self.natgrad_skipped, self.natgrad_info = self.natgrad_words[0], self.natgrad_words[1]
        sync = self.in_launch_sync()
        status = None if sync is None else sync.words[sync.status_index:sync.status_index + 1]
        recs = []
        for i, l, w, M, om, oL, scale in self._natural:
            vd = self.models[i]._layers()[l].variational_strategy._variational_distribution
            g = self._gflat[i]
            recs.append(dict(m=vd.variational_mean.data, L_S=vd.chol_variational_covar.data, g_m=g[om:om + M],
                             g_LS=g[oL:oL + M * M], scale=scale, step_count=self.natgrad_steps[w:w + 1],
                             skipped=self.natgrad_skipped[w:w + 1], info=self.natgrad_info[w:w + 1],
                             guard_info=self.infos[i], guard_status=status, guard_loss=self.losses[i, 2:3]))
        self._natgrad_table = F.NatGradSmallLayers(recs)

    def _natgrad_launch(self):
        """The second launch of a step: moves (m, L_S) of the natural-gradient layers from the flat gradients the step's launch
        has just written; on ``self.stream``, nothing in between."""
        if self._natgrad_table is not None:
            F.natgrad_small_step(self._natgrad_table, self.natgrad_gamma, self.natgrad_gamma_init, self.natgrad_warmup_steps,
                                 stream=self.stream)

    def skipped_steps(self):
        """Synchronising (one device-to-host copy): per layer, in the order of the models' layers, how many natural-gradient
        steps left it unchanged because I + 2 gamma Psi was not positive definite."""
        self.stream.synchronize()
        if self._natgrad_table is not None:
            self.skipped = self.natgrad_words[0].cpu().tolist()
        return list(self.skipped)

    # ------------------------------------------------------------------ the step
    def _launch(self, mode):
        self.kernel.launch(self, mode, self.lr, self.betas[0], self.betas[1], self.eps)

    def step(self):
        """Enqueues one step of every model on ``self.stream``."""
        self._launch(_lib.STEP_UPDATE)
        self._natgrad_launch()
        return self.losses

    def gradients(self):
        """-ELBO and its raw-parameter gradients at the current parameters, no update (``want_grad=True``): per model a dict
        parameter -> gradient tensor of its shape."""
        assert self.grads, "construct with want_grad=True"
        self._launch(_lib.STEP_GRADIENTS)
        self.stream.synchronize()
        return [{p: self.grads[i][off:off + n].reshape(p.shape) for p, off, n in segs} for i, segs in enumerate(self._segments)]

    @property
    def loss(self):
        return self.losses[:, 2]

    @property
    def kl(self):
        return self.losses[:, 1]

    # ------------------------------------------------------------------ verdicts / roll-back (as GraphedELBOStep)
    def check(self):
        """Synchronising: raises if a launch since the last check gave up an in-launch wait (functional.InLaunchWaitAbandoned),
        a Cholesky of the last step failed or a loss is not finite."""
        from ..layers.mfdgp_hidden_layer import NotPSDError
        self.stream.synchronize()
        sync = self.__dict__.get("sync")
        if sync is not None:
            sync.check("one-launch step")
        if bool((self.infos != 0).any()):
            i, l = [int(v) for v in torch.nonzero(self.infos)[0]]
            code = int(self.infos[i, l])
            if code < 0:      # (-1: a workgroup gave up waiting at an in-launch barrier; -2: the launch did not match its coupling record)
                raise F.InLaunchWaitAbandoned("one-launch step: in-launch barrier abandoned in model %d (info %d)" % (i, code))
            raise NotPSDError("K_mm not positive definite in model %d layer %d (pivot %d)" % (i, l, code))
        if not bool(torch.isfinite(self.losses).all()):
            raise FloatingPointError("non-finite ELBO")
        if self._natgrad_table is not None:      # (the natural-gradient launch waits for nothing: its info is 0 or a pivot)
            self.skipped = self.natgrad_words[0].cpu().tolist()

    def snapshot(self):
        with torch.cuda.stream(self.stream):
            self._snap = ([p.detach().clone() for m in self.models for p in m.parameters()],
                          [t.clone() for t in self.exp_avg], [t.clone() for t in self.exp_avg_sq], self.steps_done.clone(),
                          [l._rng(self.device).clone() for m in self.models for l in m._layers()])
            if self._natgrad_table is not None:
                self._snap_natgrad = (self.natgrad_steps.clone(), self.natgrad_words.clone())

    def restore(self):
        """Back to the last snapshot (parameters, optimiser state, eps streams); the in-launch counters and status start afresh."""
        self.stream.synchronize()
        sync = self.__dict__.get("sync")
        if sync is not None:
            sync.reset()
        ps, ea, eq, steps, rngs = self._snap[:5]
        with torch.no_grad(), torch.cuda.stream(self.stream):      # (ordered with the launches that follow on this stream)
            for p, s0 in zip([p for m in self.models for p in m.parameters()], ps):
                p.copy_(s0)
            for t, s0 in zip(self.exp_avg, ea):
                t.copy_(s0)
            for t, s0 in zip(self.exp_avg_sq, eq):
                t.copy_(s0)
            self.steps_done.copy_(steps)
            for layer, s0 in zip([l for m in self.models for l in m._layers()], rngs):
                layer._rng(self.device).copy_(s0)
            if self._natgrad_table is not None:
                self.natgrad_steps.copy_(self._snap_natgrad[0])
                self.natgrad_words.copy_(self._snap_natgrad[1])

    def close(self):
        """The end of this step's part of a training phase (finished, or rolled back for the layer path to continue): the
        current stream goes on after everything the step enqueued.  The object stays usable (``export_adam_state``)."""
        self.stream.synchronize()
        torch.cuda.current_stream(self.device).wait_stream(self.stream)

    def export_adam_state(self, i, optimizer):
        """Copies model i's moment estimates and step count into a FusedAdam over ``list(models[i].parameters())`` (the
        layer-path step that takes over after a failed Cholesky keeps the optimiser's memory)."""
        by_param = {id(p): (off, n) for p, off, n in self._segments[i]}
        with torch.no_grad():
            for k, p in enumerate(optimizer.params):
                if id(p) in by_param:
                    off, n = by_param[id(p)]
                    optimizer.state[k]["exp_avg"].copy_(self.exp_avg[i][off:off + n].reshape(p.shape))
                    optimizer.state[k]["exp_avg_sq"].copy_(self.exp_avg_sq[i][off:off + n].reshape(p.shape))
            optimizer.steps_done.copy_(self.steps_done[i])
            ng = getattr(optimizer, "natgrad_steps", None)
            if ng is not None and self._natgrad_table is not None:
                # a FusedNatGradAdam continues the gamma schedule where model i's layers stood (they advance together)
                mine = [w for k, _, w, _, _, _, _ in self._natural if k == i]
                if mine:
                    ng.copy_(self.natgrad_steps[mine[0]].expand_as(ng))


def _ptrs(vals):
    return (ctypes.c_void_p * len(vals))(*vals) if vals else None


class TinyConditionedStep(TinyELBOStep):
    """One iteration of the conditioned training (blackbox_mfdgp_fitter.py:245-354: fresh x~ ~ U[0,1]^(n_tilde x d), the joint
    loss over ALL surrogates, one Adam) in ONE launch instead of ~180 (mobocmf_tiny_elbo_step MOBOCMF_STEP_COUPLED: every model on [Pareto
    set | x~ | its batch], x~ drawn in the launch; after the forward the models' workgroups meet at a barrier and each forms
    the theta / omega factor gradients of its model from all models' top-layer moments), or, ``one_launch = False``, in
    3 + n_con: forward-only launch, mobocmf_cond_factors_forward for the theta factors of every constraint and for the omega
    factors on the top layers' moments, step launch with those gradients entering at the top layers' columns.
    Rows per model: the P Pareto points (objectives: scored against their column of the Pareto front, weight 1, :288-291;
    constraints: weight 0, theta factors :227-233), the x~ (weight 0, omega factors :235-243), the batch (weight num_data / B,
    KL weight 1: -elbo / B * num_data, :281-303).  One sample per row (the reference's S = 1)."""

    def __init__(self, fitter, lr, betas=(0.9, 0.999), eps=1e-8, stream=None, n_tilde=10, fixed_x_tilde=None, fixed_eps=None,
                 want_grad=False, variational_optimizer="adam", natgrad_gamma=0.1, natgrad_gamma_init=1e-4,
                 natgrad_warmup_steps=100):
        hs = fitter._handlers()
        dev = fitter.pareto_set.device
        P, d = fitter.pareto_set.shape
        Tn = n_tilde if fixed_x_tilde is None else fixed_x_tilde.shape[0]
        if Tn < 1 or P < 1:
            raise _lib.MobocmfError("TinyConditionedStep: at least one x~ point and one Pareto point (got %d, %d)" % (Tn, P))
        self.fitter, self.P, self.T = fitter, P, Tn
        self.xrng = None
        if fixed_x_tilde is None:
            self.xrng = torch.tensor([int(torch.randint(1, 2 ** 62, (), dtype=torch.int64)), 0], dtype=torch.int64, device=dev)
        prepared, self._orders = [], []
        for tag, i, h in hs:
            xb, yb, fb = h.train_dataset.tensors
            if h.mfdgp.num_samples_for_training != 1:
                raise _lib.MobocmfError("TinyConditionedStep: one training sample per row (the reference's S = 1)")
            B, top = xb.shape[0], h.num_fidelities - 1
            fv = fb.reshape(-1).to(torch.float64)
            order = torch.argsort(fv, descending=True, stable=True)
            self._orders.append(order)
            xt = torch.zeros(Tn, d, dtype=torch.float64, device=dev) if fixed_x_tilde is None else fixed_x_tilde.to(dev).double()
            z = lambda n: torch.zeros(n, dtype=torch.float64, device=dev)
            if tag == "OBJ":
                gi = fitter._global_index(h, i)
                yp, wp = fitter.pareto_front[:, gi].to(torch.float64), torch.ones(P, dtype=torch.float64, device=dev)
            else:
                yp, wp = z(P), z(P)
            e = None
            if fixed_eps is not None and fixed_eps.get((tag, i)) is not None:
                # given for the rows [batch | Pareto | x~] (fitter.conditioned_loss): into this step's [Pareto | x~ | batch sorted]
                idx = torch.cat([torch.arange(B, B + P + Tn, device=dev), order])
                e = [None if v is None else v.reshape(-1)[idx] for v in fixed_eps[(tag, i)]]
            prepared.append(dict(
                x=torch.cat([fitter.pareto_set.double(), xt, xb[order].double()], 0),
                y=torch.cat([yp, z(Tn), yb.reshape(-1)[order].double()]),
                fid=torch.cat([torch.full((P + Tn,), float(top), dtype=torch.float64, device=dev), fv[order]]),
                rows=[P + Tn + int((fv >= l).sum()) for l in range(h.num_fidelities)],
                row_weight=torch.cat([wp, z(Tn), torch.full((B,), float(h.num_data) / B, dtype=torch.float64, device=dev)]),
                kl_scale=1.0, seeds=True, seed_scale=-1.0, xrng=self.xrng, rand=(P, Tn), eps=e))
        self._roles = [(0 if tag == "OBJ" else 1) for tag, _, _ in hs]
        super().__init__([h.mfdgp for _, _, h in hs], None, None, None, None, lr, betas=betas, eps=eps, stream=stream,
                         want_grad=want_grad, prepared=prepared, variational_optimizer=variational_optimizer,
                         natgrad_gamma=natgrad_gamma, natgrad_gamma_init=natgrad_gamma_init,
                         natgrad_warmup_steps=natgrad_warmup_steps)
        # the factor launches: pointer tables into the models' top-layer moments / seed arrays, built once
        obj = [k for k, (tag, _, _) in enumerate(hs) if tag == "OBJ"]
        con = [k for k, (tag, _, _) in enumerate(hs) if tag == "CON"]
        if len(obj) > 8 or len(con) > 8:
            raise _lib.MobocmfError("TinyConditionedStep: at most 8 objectives and 8 constraints")
        self._obj, self._con = obj, con
        self.factor_losses = torch.zeros(len(con) + 1, dtype=torch.float64, device=dev)
        log_e, log_1me = float(torch.log(torch.tensor(fitter.eps, dtype=torch.float64))), \
            float(torch.log1p(torch.tensor(-fitter.eps, dtype=torch.float64)))
        thr = fitter._thresholds_on(dev).to(torch.float64).contiguous()
        front = fitter.pareto_front.to(torch.float64).contiguous()
        self._keep += [thr, front]
        mom = lambda k, r, off: self.top_moments[k][r].data_ptr() + 8 * off
        sd = lambda k, r, off: self.seeds[k][r].data_ptr() + 8 * off
        self._theta = []
        for j, k in enumerate(con):      # theta factors of constraint j at the Pareto points (columns [0, P) of its top layer)
            self._theta.append((0, 1, 1, P, None, None, _ptrs([mom(k, 0, 0)]), _ptrs([mom(k, 1, 0)]), None,
                                ctypes.c_void_p(thr.data_ptr() + 8 * j), log_1me, log_e,
                                ctypes.c_void_p(self.factor_losses[j:j + 1].data_ptr()), None, None,
                                _ptrs([sd(k, 0, 0)]), _ptrs([sd(k, 1, 0)])))
        # omega factors at the x~ (columns [P, P + T)) over all objectives and constraints
        self._omega = (len(obj), len(con), P, Tn, _ptrs([mom(k, 0, P) for k in obj]), _ptrs([mom(k, 1, P) for k in obj]),
                       _ptrs([mom(k, 0, P) for k in con]), _ptrs([mom(k, 1, P) for k in con]),
                       ctypes.c_void_p(front.data_ptr()), ctypes.c_void_p(thr.data_ptr()), log_e, log_1me,
                       ctypes.c_void_p(self.factor_losses[len(con):].data_ptr()),
                       _ptrs([sd(k, 0, P) for k in obj]), _ptrs([sd(k, 1, P) for k in obj]),
                       _ptrs([sd(k, 0, P) for k in con]), _ptrs([sd(k, 1, P) for k in con]))
        self._setup_coupling(front, thr, log_e, log_1me)

    def _setup_coupling(self, front, thr, log_e, log_1me):
        """mobocmf_tiny_coupling for the one-launch iteration (STEP_COUPLED) and every model's role in it; the descriptor table is
        uploaded again with those fields set."""
        cp = _lib.TinyCoupling()
        cp.n_obj, cp.n_con, cp.P, cp.T = len(self._obj), len(self._con), self.P, self.T
        for j, k in enumerate(self._obj):
            cp.obj_model[j] = k
            self.host[k].role, self.host[k].role_index = 0, j
        for j, k in enumerate(self._con):
            cp.con_model[j] = k
            self.host[k].role, self.host[k].role_index = 1, j
        cp.front, cp.thresholds = front.data_ptr(), thr.data_ptr()
        cp.log_eps, cp.log_1m_eps = log_e, log_1me
        cp.losses = self.factor_losses.data_ptr()
        cp.barrier, cp.status = self._barrier.data_ptr(), self._status.data_ptr()
        cp.n_models = len(self.models)
        self._coupling = torch.frombuffer(bytearray(bytes(cp)), dtype=torch.uint8).to(self.device)
        for k in range(len(self.models)):
            self.host[k].coupling = self._coupling.data_ptr()
        self._upload()

    def _factors(self):
        lib = _lib.require_device()
        st = ctypes.c_void_p(self.stream.cuda_stream)
        for a in self._theta + [self._omega]:
            _lib.check(lib.mobocmf_cond_factors_forward(*a, st), "mobocmf_cond_factors_forward")

    coupled = True
    use_graph = True      # the iteration's launch(es) replayed from one HIP graph
    one_launch = True     # the whole iteration as ONE launch (STEP_COUPLED: the factor terms formed inside, after an in-launch
    #                       barrier of the models' workgroups); False: forward-only launch + factor launches + step launch

    def _capture(self):
        """The launch(es) of an iteration captured once: every argument is static (pointers, sizes, the learning rate), x~ and
        eps come from device-side counters, so a replay IS the next iteration.  The capture pass itself executes nothing."""
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=self.stream, capture_error_mode="thread_local"):
            self._issue()
        self._graph = g

    def _issue(self):
        """The launches of one iteration, the natural-gradient launch (if any) last: a captured graph replays them all."""
        self._issue_step()
        self._natgrad_launch()

    def _issue_step(self):
        most = self.kernel.max_coupled_models
        if self.one_launch and self.T <= 256 and (most is None or len(self.models) <= most):
            try:
                self._launch(_lib.STEP_COUPLED)
                return
            except _lib.MobocmfError:
                # refused (MOBOCMF_BAD_ARG: more models than this device keeps resident at once -- the in-launch barrier
                # needs them all): nothing was enqueued; the three-launch form has no such requirement
                self.one_launch = False
        self._launch(_lib.STEP_FORWARD)
        self._factors()
        self._launch(_lib.STEP_UPDATE)

    def step(self):
        if self.use_graph:
            if self.__dict__.get("_graph") is None:
                self._capture()
            with torch.cuda.stream(self.stream):
                self._graph.replay()
        else:
            self._issue()
        return self.losses

    def gradients(self):
        assert self.grads, "construct with want_grad=True"
        self._launch(_lib.STEP_FORWARD)
        self._factors()
        self._launch(_lib.STEP_GRADIENTS)
        self.stream.synchronize()
        return [{p: self.grads[i][off:off + n].reshape(p.shape) for p, off, n in segs} for i, segs in enumerate(self._segments)]

    @property
    def loss(self):
        """The joint loss of the last iteration (:270-343): the models' terms minus the factor terms (0-dim device tensor)."""
        return self.losses[:, 2].sum() - self.factor_losses.sum()

    @property
    def x_tilde(self):
        return self.x_rows[0][self.P:self.P + self.T]

    def snapshot(self):
        super().snapshot()
        self._snap = self._snap + (None if self.xrng is None else self.xrng.clone(),)

    @property
    def _barrier(self):
        """The coupling record's arrival counter: a view of the word in front of the status word in ``in_launch_sync()``."""
        sync = self.in_launch_sync()
        return sync.words[sync.status_index - 1:sync.status_index]

    @property
    def _status(self):
        """The coupling record's status word (only ever OR'd by the launches; cleared with the counter by ``sync``)."""
        sync = self.in_launch_sync()
        return sync.words[sync.status_index:sync.status_index + 1]

    def restore(self):
        super().restore()
        xr = self._snap[-1]
        if xr is not None:
            with torch.cuda.stream(self.stream):
                self.xrng.copy_(xr)


class TinyPredictGroup(_OneLaunchGroup, PredictGroup):
    """Predictive moments of SEVERAL fitted small models at the same T test points (eval branch, the layers' fixed
    ``samples``: MFDGP.predict_for_acquisition, mfdgp.py:237-262) in ONE launch -- mobocmf_tiny_elbo_step in its forward-only
    mode -- and their gradient w.r.t. the test points in one more (STEP_INPUT_GRADIENTS): what an acquisition search evaluates
    hundreds of times against constant parameters (JESMOC_MFDGP.py:137-184).  ``moments_at(X)`` -> (n_models, 2, T * S) (T for
    fidelity 0): mean and variance of the top layer's columns, WITHOUT the likelihood noise; differentiable w.r.t. X.  The
    kernel recomputes every chain in every launch: ``freeze()`` / ``thaw()`` have nothing to do (util/predict_group.py)."""

    @classmethod
    def why_not(cls, model, fidelity, T, d, on_gpu=True, speed_rule=False):
        """``fits_predict`` with this class's ``kernel`` (``speed_rule``: see there), as None or a sentence."""
        if fits_predict(model, fidelity, T, d, speed_rule=speed_rule, kernel=cls.kernel, on_gpu=on_gpu):
            return None
        return "%s takes <= %d layers sharing M <= %d inducing inputs, d <= %d, T S <= %d columns%s, float64 parameters%s" % (
            cls.kernel.entry, _lib.TINY_MAX_LAYERS, cls.kernel.max_m, _lib.TINY_MAX_D, cls.kernel.max_predict_columns,
            " (fewer under the speed rule)" * speed_rule, " on the GPU" * on_gpu)

    def __init__(self, models, fidelity, T, d, stream=None):
        _lib.require_device()
        models = list(models)
        dev = next(models[0].parameters()).device
        self._new_table(models, dev)
        self.fidelity, self.T, self.d = fidelity, int(T), int(d)
        n, L = len(models), fidelity + 1
        self.S = models[0].num_samples_for_acquisition if L > 1 else 1
        ncol = self.T * self.S
        self.x = torch.zeros(self.T, d, dtype=torch.float64, device=dev)
        self.moments = torch.zeros(n, 2, ncol, dtype=torch.float64, device=dev)
        self.seeds = torch.zeros(n, 2, ncol, dtype=torch.float64, device=dev)
        self.gx = torch.zeros(n, self.T, d, dtype=torch.float64, device=dev)
        zrow = torch.zeros(self.T, dtype=torch.float64, device=dev)
        nofid = torch.full((self.T,), -1.0, dtype=torch.float64, device=dev)      # no row is scored: moments only
        self._keep += [zrow, nofid]
        self.info_words = []      # per model the int32 words its launches leave their Cholesky verdicts in (0: fine)
        for i, model in enumerate(models):
            reason = self.why_not(model, fidelity, self.T, d)
            if reason is None and L > 1 and model.num_samples_for_acquisition != self.S:
                reason = "S differs from the first model's"
            if reason is not None:
                raise _lib.MobocmfError("%s: model %d does not fit: %s" % (type(self).__name__, i, reason))
            Tm = self.host[i]
            desc = Descriptor.for_prediction(Tm, model, fidelity, self.T, d)
            Tm.x, Tm.y, Tm.fid = self.x.data_ptr(), zrow.data_ptr(), nofid.data_ptr()
            work = desc.allocate(self.kernel, dev)
            dummy = torch.zeros(2, desc.flat_len, dtype=torch.float64, device=dev)      # (never written: no update here)
            misc = torch.zeros(8, dtype=torch.int64, device=dev)
            out = torch.zeros(3, dtype=torch.float64, device=dev)
            self._keep += desc.keep + [work, dummy, misc, out]
            Tm.adam_m, Tm.adam_v = dummy[0].data_ptr(), dummy[1].data_ptr()
            Tm.steps_done, Tm.info, Tm.out = misc.data_ptr(), misc[4:].data_ptr(), out.data_ptr()
            self.info_words.append(misc[4:].view(torch.int32))
            Tm.top_mean, Tm.top_var = self.moments[i, 0].data_ptr(), self.moments[i, 1].data_ptr()
            Tm.seed_gmean, Tm.seed_gvar, Tm.seed_scale = self.seeds[i, 0].data_ptr(), self.seeds[i, 1].data_ptr(), 1.0
            Tm.grad = self.gx[i].data_ptr()
        self._upload()
