"""The ELBO step (zero_grad + MFDGP.forward + VariationalELBOMF + backward + Adam, blackbox_mfdgp_fitter.py:161-171)
captured once into a HIP graph and replayed.

A step of one surrogate is ~300 small launches (M x M Cholesky chain, partial reductions, elementwise glue) around a
dozen large GEMMs; issued eagerly from Python that costs ~2 ms of host time per step -- more than the GPU needs for
the small configurations (C1, C2) and half of what it needs at C3.  All library calls only enqueue work on the
caller's stream and use caller-owned memory, so the whole step is capturable; a replay costs tens of microseconds.
Fresh eps is drawn inside the graph (torch's captured Philox state advances on every replay).

GraphedMiniBatchStep is the same step on a mini-batch that the step draws on the device (csrc/minibatch.hip): one captured graph
per batch shape, a fresh batch at every replay.
"""
import os

import torch

from .. import _lib
from .. import functional as F
from ..layers.mfdgp_hidden_layer import NotPSDError


class GraphedELBOStep:
    """step() == one full-batch ELBO step on static (x, y, fidelities).  Falls back to eager with ``use_graph=False``.
    With ``prune_rows`` the rows are reordered once by descending fidelity: ``self.x`` etc. are ``x[self.row_order]``
    (``row_order`` is None when the caller's order was kept); per-row quantities map back through it.
    ``variational_optimizer="natgrad"``: every layer's q(u) moves by natural gradients (functional.FusedNatGradAdam, schedule
    ``natgrad_gamma`` / ``natgrad_gamma_init`` / ``natgrad_warmup_steps``), Adam keeps the other parameters; "adam" (default) is
    the one FusedAdam launch over all of them."""

    exchanges = False      # True in subclasses whose step has a collective between backward and update

    def __init__(self, model, elbo, x, y, fidelities, lr, betas=(0.9, 0.999), eps=1e-8, use_graph=True, stream=None,
                 warmup=3, fixed_eps=None, prune_rows=True, variational_optimizer="adam", natgrad_gamma=0.1,
                 natgrad_gamma_init=1e-4, natgrad_warmup_steps=100):
        self.elbo = elbo
        self.S = model.num_samples_for_training
        self.L = model.num_hidden_layers
        # Dead rows: the ELBO keeps, per layer, the rows of that layer's fidelity (variational_elbo_mf.py:33-38), so a row of
        # fidelity f reaches the loss through layers 0..f only.  The batch is static: order it ONCE by descending fidelity
        # (the full-batch ELBO is a sum over rows, their order is free -- the reference's loader shuffles it every epoch,
        # blackbox_mfdgp_fitter.py:35) and evaluate layer l on the prefix of rows with fidelity >= l (MFDGP.forward(rows=)).
        # Same ELBO and gradients as evaluating every layer at every row; the upper layers' panels shrink to their share.
        self.layer_rows = None
        self.row_order = None      # permutation applied to the caller's rows (None: kept): step.x == x[row_order]
        if prune_rows and self.L > F.ELBO_MAX_LAYERS:
            prune_rows = False     # pruned layer outputs need the fused ELBO (<= ELBO_MAX_LAYERS fidelities): reference layout
        if prune_rows and self.L > 1:
            fidv = fidelities.reshape(-1)
            counts = [int((fidv >= l).sum()) for l in range(self.L)]
            if counts[-1] >= 1 and counts[0] == fidv.numel():
                order = torch.argsort(fidv, descending=True, stable=True)
                x, y, fidelities = x[order].contiguous(), y[order].contiguous(), fidelities[order].contiguous()
                if fixed_eps is not None:      # given for the batch as passed in (N*S per layer): follow the rows
                    N = fidv.numel()
                    fixed_eps = [None if e is None else e.reshape(N, self.S)[order][:counts[l]].reshape(-1).contiguous()
                                 for l, e in enumerate(fixed_eps)]
                self.layer_rows = counts
                self.row_order = order
        self.x, self.y, self.fid = x, y, fidelities
        self.fixed_eps = fixed_eps     # list (eps[l] for layer l >= 1) reused every step: deterministic tests
        # "natgrad": q(u) of every layer by natural gradients, Adam on the rest.  The full-batch loss is -ELBO itself
        # (VariationalELBOMF: data terms summed over the batch - (batch / num_data) KL): scale num_data / batch
        optimizer = self._variational_optimizer(variational_optimizer, model, x.device, lr, betas, eps,
                                                float(elbo.num_data) / x.shape[0], natgrad_gamma, natgrad_gamma_init,
                                                natgrad_warmup_steps)
        if optimizer is None and os.environ.get("MOBOCMF_TORCH_ADAM"):      # A/B knob: torch's capturable Adam (seven foreach launches)
            optimizer = torch.optim.Adam(list(model.parameters()), lr=lr, betas=betas, eps=eps, capturable=True)
        self._setup(model, x.device, lr, betas, eps, use_graph, stream, optimizer=optimizer)
        if use_graph:
            self._capture(warmup)

    def _variational_optimizer(self, kind, model, device, lr, betas, eps, elbo_scale, gamma, gamma_init, warmup_steps):
        """The optimiser ``_setup`` is handed for ``variational_optimizer=kind``: None for "adam" (``_setup`` then builds the
        default FusedAdam), a FusedNatGradAdam for "natgrad".  ``elbo_scale``: what turns the step's loss into -ELBO."""
        if kind == "adam":
            return None
        if kind != "natgrad":
            raise ValueError("variational_optimizer must be 'adam' or 'natgrad' (got %r)" % (kind,))
        if self.exchanges:
            raise ValueError("variational_optimizer='natgrad' is not available for a row-sharded step (the gradients are "
                             "exchanged between backward and update); shard the surrogates over the ranks instead")
        if torch.device(device).type != "cuda":
            raise ValueError("variational_optimizer='natgrad' runs on the GPU only (CPU tensors given)")
        return F.FusedNatGradAdam(model, lr=lr, betas=betas, eps=eps, gamma=gamma, gamma_init=gamma_init,
                                  warmup_steps=warmup_steps, elbo_scale=elbo_scale)

    skipped = ()      # what the last check() read

    def skipped_steps(self):
        """Synchronising: the natural-gradient steps that left a layer unchanged, per layer ([] with Adam)."""
        fn = getattr(self.optimizer, "skipped_steps", None)
        return fn() if fn is not None else []

    def _setup(self, model, device, lr, betas, eps, use_graph, stream, optimizer=None):
        """What every captured step starts from, whatever its loss: stream, optimiser, loss / KL buffers, empty graph and
        snapshot slots, the model(s) put into the no-host-sync state, the layers' eps streams seeded.  Not every subclass uses
        all of it: the conditioned step's backward needs no ``_minus_one``, and the mini-batch step rebinds ``loss`` / ``kl`` to
        its batch shapes' buffers."""
        self.model = model
        self.use_graph = use_graph
        self.stream = stream if stream is not None else torch.cuda.Stream(device=device)
        if optimizer is None:          # one launch; step count on the device
            optimizer = F.FusedAdam(list(model.parameters()), lr=lr, betas=betas, eps=eps)
        self.optimizer = optimizer
        self.loss = torch.zeros((), dtype=torch.float64, device=device)
        self.kl = torch.zeros((), dtype=torch.float64, device=device)
        self._minus_one = torch.full((), -1.0, dtype=torch.float64, device=device)
        self.graph = self.graph_update = self._snap = None
        model.set_check_pd(False)      # no host sync inside the step; call check() when a verdict is needed
        model.clear_kl_cache()         # an older graph would pin AccumulateGrad nodes to another stream (capture-illegal)
        for layer in model._layers():  # the layers' eps streams get their seeds here, in a fixed order, eager or captured
            layer._rng(device)

    def _fwd_bwd(self):
        self.optimizer.zero_grad(set_to_none=True)
        # eps: explicit (deterministic tests) or drawn inside the layers' propagation launches (no torch generator in the
        # captured graph: its replay support costs two fill launches per replay, the draw a third)
        out = self.model(self.x, eps=self.fixed_eps, rows=self.layer_rows)
        res = self.elbo(out, self.y.T, self.fid)
        # d(-ELBO): the sign goes in as the upstream gradient (no negation node, no ones fill, no negation backward)
        res[0].backward(gradient=self._minus_one)
        self._record_loss(res, self)
        self.model.clear_kl_cache()

    def _record_loss(self, res, dst):
        """The step's -ELBO and scaled KL, from the ELBO's result ``res``, into ``dst.loss`` / ``dst.kl``."""
        neg = getattr(self.elbo, "last_neg_elbo", None)
        if neg is not None:      # the fused ELBO launch wrote -elbo next to elbo: no negation / copy launches
            dst.loss, dst.kl = neg, res[1].detach()
        else:
            torch.neg(res[0].detach(), out=dst.loss)
            dst.kl.copy_(res[1].detach())

    def _exchange(self):
        """Between backward and the update; a no-op for a surrogate that lives on one GPU (RowShardedELBOStep
        all-reduces the gradient bucket here)."""

    def _update(self):
        self.optimizer.step()

    def _eager(self):
        self._fwd_bwd()
        self._exchange()
        self._update()

    def _capture(self, warmup):
        cur = torch.cuda.current_stream(self.x.device)
        self.stream.wait_stream(cur)
        F.take_capture_pins()          # pins left behind by a capture that aborted elsewhere are not this graph's
        try:
            self._capture_on_stream(warmup)
        finally:
            # the graph replays on these buffers: they live as long as it does (also taken when the capture raised, so that
            # a failed capture cannot leak its pins into the next step's list)
            self._pinned_scratch = F.take_capture_pins()
        cur.wait_stream(self.stream)

    def _snapshot_before_warmup(self):
        """The parameters (returned) and the layers' eps streams (seed, call counter) as ``_reset_after_warmup`` puts them
        back: warm-up draws must not count either -- the first replay then draws exactly what the first eager step would
        have drawn."""
        snapshot = [p.detach().clone() for p in self.model.parameters()]
        self._rng_snapshot = [(l, l._rng(self.x.device).clone()) for l in self.model._layers()]
        return snapshot

    def _capture_on_stream(self, warmup):
        with torch.cuda.stream(self.stream):
            # the side-stream warm-up also sizes the per-stream scratch arena and the optimizer state
            snapshot = self._snapshot_before_warmup()
            for _ in range(warmup):
                self._eager()
            self._reset_after_warmup(snapshot)
            self.graph = torch.cuda.CUDAGraph()
            if not self.exchanges:
                with torch.cuda.graph(self.graph, stream=self.stream, capture_error_mode="thread_local"):
                    self._eager()
            else:       # the collective stays outside: graph | all-reduce | graph
                with torch.cuda.graph(self.graph, stream=self.stream, capture_error_mode="thread_local"):
                    self._fwd_bwd()
                self._exchange()
                self.graph_update = torch.cuda.CUDAGraph()
                with torch.cuda.graph(self.graph_update, stream=self.stream, capture_error_mode="thread_local"):
                    self._update()
                self._reset_after_warmup(snapshot)     # the capture pass above ran the exchange + nothing else for real

    def _reset_after_warmup(self, snapshot):
        with torch.no_grad():           # warm-up steps must not count as training
            for p, s0 in zip(self.model.parameters(), snapshot):
                p.copy_(s0)
            for layer, st in getattr(self, "_rng_snapshot", []):
                layer._rng(st.device).copy_(st)
            for st in self.optimizer.state.values():
                for v in st.values():
                    if torch.is_tensor(v):
                        v.zero_()
        if not self.exchanges:
            self.optimizer.zero_grad(set_to_none=True)

    def retire(self):
        """Drop the graph and this step's entry in the scratch arena (``close`` calls it when a training phase ends)."""
        self.stream.synchronize()
        self.graph = self.graph_update = None
        self._pinned_scratch = None
        F.release_scratch(self.stream)

    def close(self):
        """The end of a training phase: the models check their Choleskys on the host again, the graph goes, and the current
        stream continues after everything this step enqueued.  (The stream is idle before a subclass's ``retire`` drops its
        graphs; ``retire`` synchronises again for the callers that use it alone.)"""
        self.stream.synchronize()
        self.model.set_check_pd(True)
        self.retire()
        torch.cuda.current_stream(self.x.device).wait_stream(self.stream)

    def step(self):
        """Enqueues one step on ``self.stream``; ``self.loss`` / ``self.kl`` hold the step's -ELBO and scaled KL."""
        with torch.cuda.stream(self.stream):
            if self.graph is not None:
                self.graph.replay()
                if self.exchanges:
                    self._exchange()
                    self.graph_update.replay()
            else:
                self._eager()
        return self.loss, self.kl

    # ------------------------------------------------------------------ snapshot / fallback
    def snapshot(self):
        """Clone of parameters + optimizer state (taken at points where check() passed)."""
        with torch.cuda.stream(self.stream):
            self._snap = ([p.detach().clone() for p in self.model.parameters()],
                          [{k: (v.detach().clone() if torch.is_tensor(v) else v) for k, v in st.items()}
                           for st in self.optimizer.state.values()])

    def restore_and_go_eager(self):
        """After a failed Cholesky inside a replayed step (no host-side jitter retry is possible there): roll back to
        the last good snapshot and continue eagerly with the psd_safe_cholesky jitter ladder (check_pd=True), which is
        what the reference does at every step."""
        self.stream.synchronize()
        ps, sts = self._snap
        with torch.no_grad():
            for p, s0 in zip(self.model.parameters(), ps):
                p.copy_(s0)
            for st, s0 in zip(self.optimizer.state.values(), sts):
                for k, v in st.items():
                    if torch.is_tensor(v):
                        v.copy_(s0[k])
        self.graph = None
        self.model.set_check_pd(True)

    def check(self):
        """Synchronising: raises if a Cholesky of the last step failed or the loss is not finite."""
        self.stream.synchronize()
        for layer in self.model._layers():
            if layer._info is not None:
                pivot = F.check_info(layer._info)
                F.raise_if_abandoned(pivot, "layer %d" % layer.num_layer)
                if pivot != 0:
                    raise NotPSDError("K_mm not positive definite in layer %d" % layer.num_layer)
        self.skipped = self.skipped_steps()      # (raises when a natural-gradient factorisation abandoned an in-launch wait)
        if not bool(torch.isfinite(self.loss)):
            raise FloatingPointError("non-finite ELBO")


class _ModelGroup:
    """The models of a joint step seen as one (parameters / layers / housekeeping of GraphedELBOStep)."""

    def __init__(self, models):
        self.models = list(models)

    def parameters(self):
        for m in self.models:
            yield from m.parameters()

    def _layers(self):
        for m in self.models:
            yield from m._layers()

    def clear_kl_cache(self):
        for m in self.models:
            m.clear_kl_cache()

    def set_check_pd(self, value):
        for m in self.models:
            m.set_check_pd(value)


class GraphedConditionedStep(GraphedELBOStep):
    """One iteration of the conditioned training (blackbox_mfdgp_fitter.py:245-354: fresh x~ ~ U[0,1]^(10 x d), the joint
    loss over ALL surrogates, one Adam) captured into a HIP graph.  ``fitter.conditioned_loss`` must be capture-safe
    (no host reads); x~ is drawn inside the graph, so every replay sees new points."""

    def __init__(self, fitter, lr, betas=(0.9, 0.999), eps=1e-8, use_graph=True, stream=None, warmup=3, n_tilde=10,
                 fixed_x_tilde=None, variational_optimizer="adam", natgrad_gamma=0.1, natgrad_gamma_init=1e-4,
                 natgrad_warmup_steps=100):
        self.fitter = fitter
        self.fixed_x_tilde = fixed_x_tilde      # deterministic tests: the same x~ at every iteration
        dev = fitter.pareto_set.device
        self.device, self.d, self.n_tilde = dev, fitter.pareto_set.shape[1], n_tilde
        self.x = fitter.pareto_set            # (only its device is used by the base class)
        group = _ModelGroup(h.mfdgp for _, _, h in fitter._handlers())
        # the joint loss carries every surrogate's -ELBO whole (conditioned_loss: coefficient -num_data / B): scale 1
        optimizer = self._variational_optimizer(variational_optimizer, group.models, dev, lr, betas, eps, 1.0, natgrad_gamma,
                                                natgrad_gamma_init, natgrad_warmup_steps)
        self._setup(group, dev, lr, betas, eps, use_graph, stream, optimizer=optimizer)
        if use_graph:
            self._capture(warmup)

    def _fwd_bwd(self):
        self.optimizer.zero_grad(set_to_none=True)
        x_tilde = self.fixed_x_tilde if self.fixed_x_tilde is not None else \
            torch.rand(self.n_tilde, self.d, dtype=torch.float64, device=self.device)
        from .. import parallel
        if self.fixed_x_tilde is None and parallel.world()[1] > 1:
            parallel.broadcast_(x_tilde)      # sharded surrogates: the gathered moments must refer to the SAME points
        loss = self.fitter.conditioned_loss(x_tilde)
        loss.backward()
        self.loss.copy_(loss.detach())
        self.model.clear_kl_cache()


class _BatchShape:
    """The static buffers (and the captured graph) of one batch size of GraphedMiniBatchStep."""

    def __init__(self, rows, d, S, dev, fixed_eps, warm_step):
        self.rows = rows
        self.x = torch.zeros(rows, d, dtype=torch.float64, device=dev)
        self.y = torch.zeros(rows, 1, dtype=torch.float64, device=dev)
        self.fid = torch.zeros(rows, 1, dtype=torch.float64, device=dev)
        self.src = torch.zeros(rows, dtype=torch.int64, device=dev)
        self.loss = torch.zeros((), dtype=torch.float64, device=dev)
        self.kl = torch.zeros((), dtype=torch.float64, device=dev)
        # given per batch position for the full batch (batch_size * S per layer): the ragged batch uses its first rows * S
        self.eps = None if fixed_eps is None else [None if e is None else e.reshape(-1)[:rows * S].contiguous()
                                                   for e in fixed_eps]
        self.warm_step = warm_step      # a step count whose batch has this many rows (warm-up runs on it)
        self.graph = self.grads = None


class GraphedMiniBatchStep(GraphedELBOStep):
    """step() == one ELBO step on a mini-batch of ``batch_size`` rows that the step itself draws ON THE DEVICE
    (functional.minibatch_indices / minibatch_gather: the loader of blackbox_mfdgp_fitter.py:35 and the batch loop :156-173):
    a replay of the captured step sees a fresh batch without the host.  ``num_data // batch_size`` full batches and, when
    ``batch_size`` does not divide ``num_data``, one ragged batch make an epoch.

    Batch size, layer row counts and the ELBO's ``batch / num_data`` scale are host values baked into a capture, so the step
    holds ONE GRAPH PER SHAPE (full, ragged) over the same model, optimiser (its step count lives on the device) and sampler
    state; the host mirrors the step count to pick the graph, and the index launch checks the pick (``rows_expected``; a
    mismatch sets the sampler's status, which ``check()`` raises on).  With ``order_by_fidelity`` the batch is ordered by
    descending fidelity: the rows the upper layers do not need are contiguous, and the zero-gradient block skipping of the
    layer backward drops their tiles (the forward stays dense over the batch: no ``rows=`` pruning, the per-fidelity counts
    change from batch to batch).  ``fixed_eps`` is per batch POSITION (``batch_size * S`` per layer >= 1).

    ``src`` / ``counts`` / ``grads``: source rows of the last batch, its per-level counts #{fid >= l} and its gradients (in the
    order of ``model.parameters()``); ``epoch_loss`` / ``epoch_kl``:
    the sums over the last finished epoch, accumulated on the device."""

    def __init__(self, model, elbo, x, y, fidelities, batch_size, lr, betas=(0.9, 0.999), eps=1e-8, use_graph=True,
                 stream=None, warmup=3, fixed_eps=None, order_by_fidelity=True, sampler_state=None,
                 variational_optimizer="adam", natgrad_gamma=0.1, natgrad_gamma_init=1e-4, natgrad_warmup_steps=100):
        self.elbo = elbo
        self.S = model.num_samples_for_training
        self.L = model.num_hidden_layers
        if self.L > _lib.MINIBATCH_MAX_LEVELS:
            raise ValueError("the mini-batch step takes at most %d fidelities" % _lib.MINIBATCH_MAX_LEVELS)
        self.layer_rows = self.row_order = None
        self.x, self.y, self.fid = x.contiguous(), y.contiguous(), fidelities.contiguous()
        dev = x.device
        self.num_data = N = x.shape[0]
        if int(elbo.num_data) != N:
            raise ValueError("the ELBO scales the KL by batch / num_data: elbo.num_data must be the number of rows of x")
        self.batch_size = B = max(1, min(int(batch_size), N))
        self.nb = (N + B - 1) // B
        self.order_by_fidelity = bool(order_by_fidelity)
        self.fixed_eps = fixed_eps
        # (a mini-batch's loss is (rows / num_data) times an unbiased estimate of -ELBO: _update sets the batch's own scale)
        optimizer = self._variational_optimizer(variational_optimizer, model, dev, lr, betas, eps, float(N) / B, natgrad_gamma,
                                                natgrad_gamma_init, natgrad_warmup_steps)
        self._setup(model, dev, lr, betas, eps, use_graph, stream, optimizer=optimizer)
        if sampler_state is None:      # drawn once from torch's CPU generator, after the layers' streams (as layer._rng)
            sampler_state = F.minibatch_state(int(torch.randint(1, 2 ** 62, (), dtype=torch.int64)), dev)
        self.state = sampler_state
        self._host_step = int(self.state[1])      # the host's mirror of the device step count: which graph to replay
        d = x.shape[1]
        ragged = N % B
        self.shapes = [_BatchShape(B, d, self.S, dev, fixed_eps, 0)]
        if ragged:
            self.shapes.append(_BatchShape(ragged, d, self.S, dev, fixed_eps, self.nb - 1))
        self._shape = self.shapes[0]
        self.counts = torch.zeros(_lib.MINIBATCH_MAX_LEVELS, dtype=torch.int64, device=dev)
        self.sums = torch.zeros(4, dtype=torch.float64, device=dev)
        self.epoch_loss, self.epoch_kl = self.sums[2], self.sums[3]
        self.loss, self.kl, self.src = self._shape.loss, self._shape.kl, self._shape.src
        self.stream.wait_stream(torch.cuda.current_stream(dev))
        if use_graph:
            self._capture(warmup)

    def _update(self):
        if hasattr(self.optimizer, "set_elbo_scale"):      # a host value, baked into this shape's graph
            self.optimizer.set_elbo_scale(float(self.num_data) / self._shape.rows)
        self.optimizer.step()

    def _shape_for(self, step):
        last = len(self.shapes) > 1 and step % self.nb == self.nb - 1
        return self.shapes[1] if last else self.shapes[0]

    def _fwd_bwd(self):
        b = self._shape
        self.optimizer.zero_grad(set_to_none=True)
        F.minibatch_indices(self.state, self.fid, self.batch_size, self.L, b.src, self.counts, self.order_by_fidelity)
        F.minibatch_gather(self.state, b.src, self.x, self.y, self.fid, b.x, b.y, b.fid)
        out = self.model(b.x, eps=b.eps)      # reference layout: every layer over the whole batch
        res = self.elbo(out, b.y.T, b.fid)
        res[0].backward(gradient=self._minus_one)
        b.grads = [p.grad for p in self.model.parameters()]      # under capture: static, rewritten by every replay of this shape
        self._record_loss(res, b)
        F.minibatch_accumulate(self.state, self.num_data, self.batch_size, b.loss, b.kl, self.sums)
        self.model.clear_kl_cache()

    def _capture_on_stream(self, warmup):
        with torch.cuda.stream(self.stream):
            snapshot = self._snapshot_before_warmup()
            state0, sums0 = self.state.clone(), self.sums.clone()
            # BOTH shapes warm up and are captured before the first real step (_reset_after_warmup zeroes the optimiser
            # state); a shape warms up on a step count whose batch has its rows, and the sampler state is put back afterwards
            # like the layers' eps streams
            for b in self.shapes:
                warm = torch.tensor([int(state0[0]), b.warm_step, 0], dtype=torch.int64, device=self.x.device)
                self._shape = b
                for _ in range(warmup):
                    self.state.copy_(warm)
                    self._eager()
            self._reset_after_warmup(snapshot)
            self.state.copy_(state0)
            self.sums.copy_(sums0)
            for b in self.shapes:
                self._shape = b
                b.graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(b.graph, stream=self.stream, capture_error_mode="thread_local"):
                    self._eager()
            self.graph = self.shapes[0].graph

    def retire(self):
        for b in self.shapes:
            b.graph = None
        super().retire()

    def step(self):
        """Enqueues one mini-batch step on ``self.stream``; ``self.loss`` / ``self.kl`` / ``self.src`` are the batch's."""
        b = self._shape_for(self._host_step)
        with torch.cuda.stream(self.stream):
            if self.graph is not None:
                b.graph.replay()
            else:          # the same launches, uncaptured
                self._shape = b
                self._eager()
        self._host_step += 1
        self.loss, self.kl, self.src, self.grads = b.loss, b.kl, b.src, b.grads
        return self.loss, self.kl

    def snapshot(self):
        super().snapshot()
        with torch.cuda.stream(self.stream):      # with the sampler: a rollback replays the same batches
            self._snap_sampler = (self.state.clone(), self.sums.clone(), self._host_step)

    def restore_and_go_eager(self):
        state, sums, self._host_step = self._snap_sampler
        with torch.cuda.stream(self.stream):      # the copies go where the next steps run
            super().restore_and_go_eager()
            self.state.copy_(state)
            self.sums.copy_(sums)

    def check(self):
        self.stream.synchronize()
        F.minibatch_check(self.state)
        super().check()
