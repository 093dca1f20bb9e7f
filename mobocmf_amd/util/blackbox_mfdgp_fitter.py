"""Trainer/orchestrator -- host mirror of mobocmf/util/blackbox_mfdgp_fitter.py (unconditioned training:
``MFDGPHandler`` :22-39, ``BlackBoxMFDGPFitter.__init__`` :43-81, ``initialize_mfdgp`` :84-115,
``_train_mfdgp`` :117-152, ``train_mfdgps`` :154-178; the ELBO step is :161-171).

Conditioned training (:245-354) and Pareto sampling of posterior function samples (:181-225, row N2)
are mirrored below over the same HIP path.

MI355X additions: ``device`` (models and data live on the GPU), ``num_inducing`` / ``num_samples_for_training``
pass-through, and surrogate sharding over ranks (one process per GPU, see mobocmf_amd.parallel).

Which GPyTorch branch the training batch takes: the reference trains on ``DataLoader(..., shuffle=True)`` (:35), so with
its default Z = x_train the full batch is a random PERMUTATION of Z and ``torch.equal(x, Z)`` is false: layer 0 goes through
the general path (mu = K_nm (K_mm + eps I)^-1 m, not m itself).  Both trainers here do the same: the eager one iterates the
shuffling loader, the HIP-graph one captures the step on a fixed non-identity permutation of the rows (the full-batch
loss does not depend on the row order).
"""
import sys
import warnings
from copy import deepcopy

import numpy as np
import torch
from torch.utils.data import DataLoader, TensorDataset

from .. import _lib, parallel
from .. import functional as F
from ..gp import MultivariateNormal as MVN
from ..layers.mfdgp_hidden_layer import NotPSDError
from ..mlls.variational_elbo_mf import VariationalELBOMF
from ..models.mfdgp import MFDGP, TL
from . import coop_step, graphed_step, tiny_step

ITER_PRINT = 1000

REDO_EAGERLY, HAND_OVER = "redo eagerly", "hand over"      # what run_verified does after a failed verdict


def run_verified(steps, num_iters, on_failure, labels, unit, report=None):
    """The training loop of every captured and one-launch path: ``num_iters`` iterations of the step objects in ``steps``
    (GraphedELBOStep and its subclasses, TinyELBOStep and its: ``step / check / snapshot / restore... / close``), their state
    verified on the host every ITER_PRINT iterations and after the last one -- nothing in between reads the device.

    An iteration is ``g.nb`` steps of every ``g`` (1 where a step object has no ``nb``), the objects advancing in lockstep.
    At a verification each object in turn is checked (``check`` synchronises its stream), snapshotted when it passed and
    then reported (``report(i, j, g)``, None: silent); ``last_good`` is kept per object, so per surrogate where ``steps`` holds
    one object per surrogate and per group where it holds one object for all of them.  When ``check`` raises NotPSDError or
    FloatingPointError -- a replayed graph or a launch without the host in it cannot retry with more jitter -- the object goes
    back to its last verified state and, with ``on_failure``
      REDO_EAGERLY  redoes the iterations since then itself (``restore_and_go_eager``: per-step jitter ladder, as the reference
                    at every step) and stays eager for the rest of the phase;
      HAND_OVER     is closed and returned with the number of iterations that stand: the caller continues on another path.
                    Takes a single object: others would be left where the iteration had taken them.
    ``labels[j]`` opens object j's warning, ``unit`` names the iterations in it.  Returns (iterations completed, the object that
    handed over or None); when all were completed every object has been closed."""
    assert on_failure != HAND_OVER or len(steps) == 1
    nbs = [getattr(g, "nb", 1) for g in steps]
    last_good = [-1] * len(steps)          # last iteration whose state was verified
    skipped_seen = [0] * len(steps)
    for g in steps:
        g.snapshot()
    for i in range(num_iters):
        for k in range(max(nbs, default=0)):
            for g, nb in zip(steps, nbs):
                if k < nb:
                    g.step()
        if (i % ITER_PRINT) == 0 or (i + 1) == num_iters:
            for j, (g, nb) in enumerate(zip(steps, nbs)):
                try:
                    g.check()
                except (NotPSDError, FloatingPointError) as err:
                    redo = i - last_good[j]
                    msg = "%s%s -- rolling back %d %s" % (labels[j], err, redo, unit)
                    if on_failure == HAND_OVER:
                        warnings.warn(msg + "; the layer path continues")
                        g.restore()
                        g.close()
                        return last_good[j] + 1, g
                    warnings.warn(msg + " and redoing them eagerly")
                    g.restore_and_go_eager()
                    for _ in range(redo * nb):
                        g.step()
                    g.check()
                g.snapshot()
                last_good[j] = i
                total = sum(getattr(g, "skipped", ()))      # natural-gradient steps that left a layer's q(u) unchanged (read by check)
                if total > skipped_seen[j]:
                    print("%s%d natural-gradient steps skipped so far (I + 2 gamma Psi not positive definite)" % (labels[j], total))
                    skipped_seen[j] = total
                if report is not None:
                    report(i, j, g)
    for g in steps:
        g.close()
    return num_iters, None


def _prod(t, dim):
    """Product over a (short) dimension as a chain of multiplications: torch.prod's backward counts zeros on the host
    (.item()), which a stream capture forbids."""
    parts = t.unbind(dim)
    out = parts[0]
    for p in parts[1:]:
        out = out * p
    return out


def _ncdf(z):
    """Standard normal cdf (the reference uses torch.distributions Normal(0, 1).cdf, :18)."""
    return 0.5 * (1.0 + torch.erf(z * 0.7071067811865476))


class MFDGPHandler:

    MAX_TRIES_FOR_FEASIBLE_GRID = 50

    def __init__(self, x_train, y_train, fidelities_train, num_fidelities, batch_size, type_lengthscale,
                 previously_trained_model=None, init_params_to_prior_and_fix_them=False,
                 use_only_highest_fidelity=False, device="cuda", warm_start="hypers", **model_kwargs):
        if model_kwargs.get("inducing_selection", "first") != "first":
            model_kwargs.setdefault("inducing_device", device)     # the selection runs where the model will live
        self.mfdgp = MFDGP(x_train, y_train, fidelities_train, num_fidelities=num_fidelities,
                           type_lengthscale=type_lengthscale, previously_trained_model=previously_trained_model,
                           use_only_highest_fidelity=use_only_highest_fidelity,
                           init_params_to_prior_and_fix_them=init_params_to_prior_and_fix_them, warm_start=warm_start,
                           **model_kwargs)
        self.mfdgp.double()  # float64 end to end, as the reference (:32)
        self.mfdgp.to(device)
        self.elbo = VariationalELBOMF(self.mfdgp, x_train.shape[-2], num_fidelities=num_fidelities)
        dev = torch.device(device)
        self.train_dataset = TensorDataset(x_train.double().to(dev), y_train.double().to(dev),
                                           fidelities_train.double().to(dev))
        self.batch_size = batch_size
        self.train_loader = DataLoader(self.train_dataset, batch_size=batch_size, shuffle=True)
        self.iter_train_loader = None
        self.num_data = x_train.shape[0]
        self.num_fidelities = num_fidelities
        self.global_index = None       # position among ALL objectives (or constraints) when surrogates are sharded over ranks
        # the captured mini-batch step's sampler: int64 {seed, step, status} on the device, made at the first training phase and
        # kept across phases; ``minibatch_seed`` (None: drawn from torch's CPU generator) fixes its seed
        self.minibatch_seed = None
        self.minibatch_state = None


class BlackBoxMFDGPFitter:

    def __init__(self, num_fidelities, batch_size, lr_1=0.003, lr_2=0.001, num_epochs_1=5000, num_epochs_2=15000,
                 pareto_set_size=50, opt_grid_size=1000, eps=1e-8, decoupled_evals=False,
                 type_lengthscale=TL.MEDIAN, device="cuda", pareto_refine="slsqp", variational_optimizer="adam",
                 natgrad_gamma=0.1, natgrad_gamma_init=1e-4, natgrad_warmup_steps=100, natgrad_one_launch=False,
                 pareto_search="grid", pareto_evolve_population=128, pareto_evolve_generations=100,
                 learn_inducing_locations=False, **model_kwargs):
        # True: every surrogate owns one trainable Z_x (MFDGP(learn_inducing_locations=True)); it trains through the captured
        # layer-path steps (the one-launch steps treat Z as a constant) and belongs to the Adam group
        self.learn_inducing_locations = bool(learn_inducing_locations)
        if self.learn_inducing_locations:
            model_kwargs["learn_inducing_locations"] = True
        if pareto_refine not in ("slsqp", "device"):
            raise ValueError("pareto_refine must be 'slsqp' or 'device' (got %r)" % (pareto_refine,))
        if pareto_search not in ("grid", "evolve"):
            raise ValueError("pareto_search must be 'grid' or 'evolve' (got %r)" % (pareto_search,))
        if not 4 <= int(pareto_evolve_population) <= 512 or int(pareto_evolve_population) % 2:
            raise ValueError("pareto_evolve_population must be even, 4..512 (got %r)" % (pareto_evolve_population,))
        if int(pareto_evolve_generations) < 1:
            raise ValueError("pareto_evolve_generations must be >= 1")
        # MOOP's search: the random grid | NSGA-II on the GPU from the grid's rows (util/pareto_evolve.py)
        self.pareto_search = pareto_search
        self.pareto_evolve_population = int(pareto_evolve_population)
        self.pareto_evolve_generations = int(pareto_evolve_generations)
        if variational_optimizer not in ("adam", "natgrad"):
            raise ValueError("variational_optimizer must be 'adam' or 'natgrad' (got %r)" % (variational_optimizer,))
        if natgrad_one_launch and variational_optimizer != "natgrad":
            raise ValueError("natgrad_one_launch=True needs variational_optimizer='natgrad' (got %r)" % (variational_optimizer,))
        # "natgrad": q(u) of every layer moves by natural gradients inside the captured layer-path steps (both training phases
        # and the conditioned fit), Adam keeps the other parameters; the one-launch steps are taken only with
        # natgrad_one_launch=True (their step plus one natural-gradient launch for all layers, util/tiny_step.py)
        self.variational_optimizer = variational_optimizer
        self.natgrad_one_launch = bool(natgrad_one_launch)
        self.natgrad_gamma, self.natgrad_gamma_init = natgrad_gamma, natgrad_gamma_init
        self.natgrad_warmup_steps = natgrad_warmup_steps
        self.pareto_refine = pareto_refine      # MOOP's refine: host SLSQP | the one-launch refinement on the GPU
        self.num_obj = 0
        self.num_con = 0
        self.models_uncond_trained = False
        self.mfdgp_handlers_objs = {}
        self.mfdgp_handlers_cons = {}
        self.thresholds_cons = torch.tensor([], dtype=torch.double)
        self.x_train = None
        self.objs_train = torch.tensor([], dtype=torch.double)
        self.cons_train = torch.tensor([], dtype=torch.double)
        self.num_fidelities = num_fidelities
        self.batch_size = batch_size
        self.points_to_sample = batch_size
        self.lr_1, self.lr_2 = lr_1, lr_2
        self.num_epochs_1, self.num_epochs_2 = num_epochs_1, num_epochs_2
        self.pareto_set_size = pareto_set_size
        self.opt_grid_size = opt_grid_size
        self.eps = eps
        self.decoupled_evals = decoupled_evals
        self.type_lengthscale = type_lengthscale
        self.device = device
        self.model_kwargs = model_kwargs
        self.verbose = True
        self.thresholds_cons_global = None      # sharded surrogates: thresholds of ALL constraints, global order

    def set_global_constraint_thresholds(self, thresholds):
        """Surrogates sharded over ranks (mobocmf_amd.parallel): the omega factors (:235-243) see every constraint of the
        problem, so each rank needs the whole threshold vector in global constraint order (``global_index`` of
        ``initialize_mfdgp``).  Single process: not needed (the local vector is the whole one)."""
        self.thresholds_cons_global = torch.as_tensor(thresholds, dtype=torch.double).reshape(-1)
        self._thr_cache = None

    def initialize_mfdgp(self, x_train, y_train, fidelities, blackbox_name, threshold_constraint=0.0,
                         is_constraint=False, previously_trained_model=None,
                         init_params_to_prior_and_fix_them=False, use_only_highest_fidelity=False, global_index=None,
                         warm_start="hypers"):
        """``global_index`` (sharded surrogates only): this black-box's position among ALL objectives -- the column of the
        Pareto front it is conditioned on -- or among ALL constraints; default: its position on this rank.
        ``warm_start`` (with ``previously_trained_model``): "hypers" carries over the kernel hyper-parameters and the fixed
        samples, "posterior" every layer's q(u) and the noise as well (``MFDGP``, util/warm_start.py): a refit on appended
        rows then starts from the previous optimum and needs no phase 1 (``num_epochs_1 = 0``)."""
        if getattr(self, "decoupled_evals", False):
            # every black-box has its own inputs: x_train is the union of the rows seen so far, in first-seen order without
            # duplicates -- only MOOP's extra grid points and the input hash of the seeded exchange; the (unused) joint
            # observation tables have no meaning
            self._add_inputs(x_train)
            self.objs_train = self.cons_train = None
        elif self.x_train is None:
            self.x_train = x_train
        else:
            assert torch.equal(self.x_train, x_train), "The inputs for this new mfdgp do not match with inputs for " \
                "previous mfdgp models. This class is not currently prepared for a decoupled evaluation setting."
        handler = MFDGPHandler(x_train, y_train, fidelities, self.num_fidelities, self.batch_size,
                               type_lengthscale=self.type_lengthscale,
                               previously_trained_model=previously_trained_model,
                               init_params_to_prior_and_fix_them=init_params_to_prior_and_fix_them,
                               use_only_highest_fidelity=use_only_highest_fidelity, device=self.device,
                               warm_start=warm_start, **self.model_kwargs)
        handler.global_index = global_index
        if is_constraint:
            if self.cons_train is not None:
                self.cons_train = torch.cat((self.cons_train, y_train.cpu().double()), 1)
            self.mfdgp_handlers_cons[blackbox_name] = handler
            self.thresholds_cons = torch.cat((self.thresholds_cons, torch.tensor([threshold_constraint]).double()), 0)
            self.num_con += 1
        else:
            if self.objs_train is not None:
                self.objs_train = torch.cat((self.objs_train, y_train.cpu().double()), 1)
            self.mfdgp_handlers_objs[blackbox_name] = handler
            self.num_obj += 1

    def _add_inputs(self, x_train):
        """``decoupled_evals``: appends the rows of ``x_train`` that ``self.x_train`` does not hold yet, in their order."""
        seen = set() if self.x_train is None else {tuple(r) for r in self.x_train.detach().cpu().double().tolist()}
        keep = []
        for i, r in enumerate(x_train.detach().cpu().double().tolist()):
            if tuple(r) not in seen:
                seen.add(tuple(r))
                keep.append(i)
        new = x_train[torch.tensor(keep, dtype=torch.int64, device=x_train.device)]
        self.x_train = new if self.x_train is None else torch.cat([self.x_train, new.to(self.x_train)], 0)

    def _natgrad(self):
        return getattr(self, "variational_optimizer", "adam") == "natgrad"

    def _one_launch_allowed(self):
        """The one-launch steps are tried first: always with Adam, with natural gradients only on request."""
        if getattr(self, "learn_inducing_locations", False):      # TinyELBOStep / CoopELBOStep hold Z_x as a constant
            return False
        return not self._natgrad() or getattr(self, "natgrad_one_launch", False)

    def _optimizer_kwargs(self):
        """The captured steps' optimiser keywords."""
        if not self._natgrad():
            return {}
        return dict(variational_optimizer="natgrad", natgrad_gamma=self.natgrad_gamma, natgrad_gamma_init=self.natgrad_gamma_init,
                    natgrad_warmup_steps=self.natgrad_warmup_steps)

    def _handlers(self):
        return [("OBJ", n, h) for n, h in enumerate(self.mfdgp_handlers_objs.values())] + \
               [("CON", n, h) for n, h in enumerate(self.mfdgp_handlers_cons.values())]

    def get_model(self, blackbox_name, is_constraint=False):
        d = self.mfdgp_handlers_cons if is_constraint else self.mfdgp_handlers_objs
        return d[blackbox_name].mfdgp

    def _train_mfdgp(self, func_update_model, fix_variational_hypers, num_epochs, lr):
        opts = []
        for _, _, h in self._handlers():
            h.mfdgp.fix_variational_hypers(fix_variational_hypers)
            opts.append(F.FusedAdam(list(h.mfdgp.parameters()), lr=lr))      # torch.optim.Adam's update in one launch
        for (tag, n, h), optimizer in zip(self._handlers(), opts):
            for i in range(num_epochs):
                loss_iter, kl_iter = func_update_model(h.mfdgp, h.elbo, optimizer, h.train_loader)
                if self.verbose and ((i % ITER_PRINT) == 0 or (i + 1) == num_epochs):
                    print("[%s: " % tag, n, "] Epoch:", i, "/", num_epochs, ". Avg. Neg. ELBO per epoch:",
                          loss_iter.item(), "\t KL per epoch:", kl_iter.item())
                    sys.stdout.flush()

    @staticmethod
    def update_model(model, elbo, optimizer, train_loader):
        """One epoch = the reference's ``_update_model`` closure (:156-173); one ELBO step per batch."""
        loss_iter = 0.0
        kl_iter = 0.0
        for (x_batch, y_batch, fidelities) in train_loader:
            optimizer.zero_grad()
            output = model(x_batch)
            res = elbo(output, y_batch.T, fidelities)
            loss, kl = -res[0], res[1]
            loss.backward()
            optimizer.step()
            loss_iter += loss.detach()
            kl_iter += kl.detach()
        return loss_iter, kl_iter

    def _stream_for(self, slot, device):
        """One HIP stream per surrogate slot, created once per fitter and reused by every training phase.  Replaying a
        captured step on a stream created LATER in the process is ~1.5x slower at the sizes where the step is bound by
        graph-node dispatch (0.37 vs 0.55 ms per Forrester step, measured: the first streams get hardware queues of their
        own), and torch hands stream handles out of a small pool anyway."""
        pool = self.__dict__.setdefault("_step_streams", {})
        key = (str(device), slot)
        if key not in pool:
            pool[key] = torch.cuda.Stream(device=device)
        return pool[key]

    def __getstate__(self):
        state = self.__dict__.copy()
        state.pop("_step_streams", None)       # streams are process-local: never copied / pickled (copy_uncond, dill)
        state.pop("_thr_cache", None)
        return state

    @staticmethod
    def shuffled_rows(n, device):
        """One draw of the loader's shuffle (:35), never the identity for n > 1: the row order the captured step keeps.
        (An identity draw -- probability 1/n! in the reference -- would send layer 0 through GPyTorch's equal-inputs
        shortcut; the general branch is what the reference's training executes.)"""
        perm = torch.randperm(n)
        if n > 1 and bool((perm == torch.arange(n)).all()):
            perm = torch.roll(perm, 1)
        return perm.to(device)

    def _train_mfdgp_graphed(self, fix_variational_hypers, num_epochs, lr):
        """Full-batch fast path: every surrogate's ELBO step is captured into a HIP graph (mobocmf_amd.util.graphed_step)
        and the independent surrogates advance in lockstep on separate streams (the reference loops over them one
        after the other, :134-152; they share nothing, so the result only differs in which N(0,1) draws each gets).
        The rows are shuffled once (see the module docstring): the step runs GPyTorch's general branch, as the
        reference's shuffled batches do."""
        # the reference's own sizes (M = N = tens of points): every surrogate's whole step in ONE launch per epoch
        done, tiny = (0, None)
        if self._one_launch_allowed():
            done, tiny = self._train_mfdgp_tiny(fix_variational_hypers, num_epochs, lr)
        if done >= num_epochs:
            return
        num_epochs -= done
        steps = []
        for slot, (tag, n, h) in enumerate(self._handlers()):
            h.mfdgp.fix_variational_hypers(fix_variational_hypers)
            x, y, fid = h.train_dataset.tensors
            perm = self.shuffled_rows(x.shape[0], x.device)
            steps.append(graphed_step.GraphedELBOStep(h.mfdgp, h.elbo, x[perm].contiguous(), y[perm].contiguous(),
                                                      fid[perm].contiguous(), lr=lr, stream=self._stream_for(slot, x.device),
                                                      **self._optimizer_kwargs()))
            if tiny is not None:      # a Cholesky failed in the one-launch step: this path (jitter ladder) takes over its state
                tiny.export_adam_state(slot, steps[-1].optimizer)
        self._run_layer_path(steps, num_epochs, lambda g: (g.loss, g.kl))

    def _run_layer_path(self, steps, num_epochs, loss_kl):
        """run_verified over one step object per surrogate, each redoing its own lost epochs; ``loss_kl(g)``: what to print."""
        hs = self._handlers()
        report = lambda i, j, g: self._print_epoch(hs[j][0], hs[j][1], i, num_epochs, *loss_kl(g))
        run_verified(steps, num_epochs, REDO_EAGERLY, ["%s %d: " % (tag, n) for tag, n, _ in hs], "epochs",
                     report if self.verbose else None)

    @staticmethod
    def _print_epoch(tag, n, i, num_epochs, loss, kl):
        print("[%s: " % tag, n, "] Epoch:", i, "/", num_epochs, ". Avg. Neg. ELBO per epoch:", loss.item(),
              "\t KL per epoch:", kl.item())
        sys.stdout.flush()

    use_tiny_step = True      # False: always the layer path (A/B, tests)

    def _train_mfdgp_tiny(self, fix_variational_hypers, num_epochs, lr):
        """The training phase through mobocmf_tiny_elbo_step (util/tiny_step.py) when EVERY surrogate fits it: one launch
        per epoch for all of them.  Returns (epochs completed, step object or None): fewer than ``num_epochs`` when the
        surrogates do not fit (0, None) or when a Cholesky failed -- the state is then rolled back to the last verified epoch
        and the layer path, which can retry with more jitter as the reference does at every step, continues from there."""
        hs = self._handlers()
        if not self.use_tiny_step or not hs:
            return 0, None
        for _, _, h in hs:
            h.mfdgp.fix_variational_hypers(fix_variational_hypers)
        data = [h.train_dataset.tensors for _, _, h in hs]
        # M <= 32 and narrow panels: one workgroup per surrogate (csrc/tiny_step.hip); up to M = 128: several workgroups per
        # surrogate, MFMA products (csrc/coop_step.hip); beyond that, or for wide panels, the layer path
        if all(x.is_cuda and tiny_step.eligible(h.mfdgp, x, fid) for (_, _, h), (x, _, fid) in zip(hs, data)):
            cls = tiny_step.TinyELBOStep
        elif all(x.is_cuda and coop_step.worthwhile(h.mfdgp, x, fid) for (_, _, h), (x, _, fid) in zip(hs, data)):
            cls = coop_step.CoopELBOStep
        else:
            return 0, None
        dev = data[0][0].device
        step = cls([h.mfdgp for _, _, h in hs], [h.num_data for _, _, h in hs], [t[0] for t in data],
                   [t[1] for t in data], [t[2] for t in data], lr=lr, stream=self._stream_for(0, dev),
                   **self._optimizer_kwargs())
        step.stream.wait_stream(torch.cuda.current_stream(dev))

        def report(i, _, step):
            out = step.losses.cpu()
            for k, (tag, n, _) in enumerate(hs):
                self._print_epoch(tag, n, i, num_epochs, out[k, 2], out[k, 1])

        return run_verified([step], num_epochs, HAND_OVER, [""], "epochs", report if self.verbose else None)[0], step

    def _train_mfdgp_minibatch(self, fix_variational_hypers, num_epochs, lr):
        """batch_size < num_data on a GPU: every surrogate's mini-batch step is captured (GraphedMiniBatchStep: the batch is
        drawn, ordered and gathered on the device inside the graph) and the surrogates advance in lockstep on their streams.
        An epoch is ``nb = ceil(num_data / batch_size)`` steps, as in the reference's loader loop (:156-173); each surrogate
        has its own sampler state, so the batches it sees do not depend on which other surrogates train next to it.
        Handlers share ``batch_size`` and the inputs, so either all of them are full-batch or none is; a handler whose batch
        happened to cover its data would run here as one batch per epoch (nb = 1), correct but without the dead-row pruning
        of the full-batch captured step."""
        steps = []
        for slot, (tag, n, h) in enumerate(self._handlers()):
            h.mfdgp.fix_variational_hypers(fix_variational_hypers)
            x, y, fid = h.train_dataset.tensors
            for layer in h.mfdgp._layers():     # the layers' seeds first, then the sampler's: the order the step itself uses
                layer._rng(x.device)
            if h.minibatch_state is None or h.minibatch_state.device != x.device:
                seed = h.minibatch_seed if h.minibatch_seed is not None else int(torch.randint(1, 2 ** 62, (), dtype=torch.int64))
                h.minibatch_state = F.minibatch_state(seed, x.device)
            steps.append(graphed_step.GraphedMiniBatchStep(h.mfdgp, h.elbo, x, y, fid, h.batch_size, lr=lr,
                                                           stream=self._stream_for(slot, x.device),
                                                           sampler_state=h.minibatch_state, **self._optimizer_kwargs()))
        # a rollback takes the sampler's state back too, so the redone epochs draw the same batches again
        self._run_layer_path(steps, num_epochs, lambda g: (g.epoch_loss, g.epoch_kl))

    def train_mfdgps(self, use_graphs=None):
        """2-phase Adam schedule of the reference (:175-176).  ``use_graphs`` (default: on a GPU) selects the HIP-graph fast
        path: the full-batch captured step when every handler trains on the full batch (as all the reference's examples
        do), the captured mini-batch step (batches drawn on the device) when ``batch_size < num_data``.  ``use_graphs=False``
        keeps the reference's host loader."""
        full_batch = all(h.batch_size >= h.num_data for _, _, h in self._handlers())
        if use_graphs is None:
            use_graphs = str(self.device).startswith("cuda")
        if self._natgrad() and not use_graphs:
            raise ValueError("variational_optimizer='natgrad' lives in the captured steps on the GPU: not with use_graphs=False "
                             "(the host loader) or CPU tensors")
        # a fitter whose models all start from a previous posterior and that has no phase 1 builds nothing for it
        warm = all(getattr(h.mfdgp, "warm_start", "hypers") == "posterior" for _, _, h in self._handlers())
        skip_1 = use_graphs and warm and self.num_epochs_1 <= 0 and bool(self._handlers())
        if use_graphs and full_batch:
            if not skip_1:
                self._train_mfdgp_graphed(True, self.num_epochs_1, self.lr_1)
            self._train_mfdgp_graphed(False, self.num_epochs_2, self.lr_2)
        elif use_graphs:      # the one-launch steps (TinyELBOStep / CoopELBOStep) are full-batch kernels: not taken here
            if not skip_1:
                self._train_mfdgp_minibatch(True, self.num_epochs_1, self.lr_1)
            self._train_mfdgp_minibatch(False, self.num_epochs_2, self.lr_2)
        else:
            self._train_mfdgp(self.update_model, fix_variational_hypers=True, num_epochs=self.num_epochs_1, lr=self.lr_1)
            self._train_mfdgp(self.update_model, fix_variational_hypers=False, num_epochs=self.num_epochs_2, lr=self.lr_2)
        self.models_uncond_trained = True

    # ------------------------------------------------------------------ Pareto solution of posterior samples (row N2)
    def _sample_and_store_pareto_solution(self, nFeatures=500, generator=None, rng=None):
        """One posterior function sample per black-box (top layer), then the feasible Pareto set of the sampled
        problem on a random grid + the training inputs (blackbox_mfdgp_fitter.py:181-216)."""
        from .moop import MOOP, NotFeasiblePoints
        # the same function for the same generator, as tensors MOOP can refine / evolve on the GPU
        if self.pareto_refine == "device" or self.pareto_search == "evolve":
            from ..layers.rff import sample_chain_from_posterior
            draw = lambda h: sample_chain_from_posterior(h.mfdgp, nFeatures=nFeatures, generator=generator)
        else:
            draw = lambda h: h.mfdgp.sample_function_from_each_layer(nFeatures=nFeatures, generator=generator)[-1]
        samples_objs = [draw(h) for h in self.mfdgp_handlers_objs.values()]
        inputs = self.x_train.detach().cpu().double().numpy()
        feasible = -1.0 * self.thresholds_cons.numpy()
        optimizer = None
        for _ in range(MFDGPHandler.MAX_TRIES_FOR_FEASIBLE_GRID):
            samples_cons = [draw(h) for h in self.mfdgp_handlers_cons.values()]
            optimizer = MOOP(samples_objs, samples_cons, input_dim=inputs.shape[1],
                             grid_size=self.opt_grid_size * inputs.shape[1], pareto_set_size=self.pareto_set_size,
                             feasible_values=feasible, rng=rng, refine=self.pareto_refine, **self._moop_search_kwargs())
            res = optimizer.compute_pareto_solution_from_samples(inputs)
            if res is not None:
                break
        else:   # no feasible grid point in any try: settle for the least infeasible points of the last samples
            res = optimizer.compute_pareto_solution_from_samples(inputs, allow_negative_constraints=True)
            if res is None:
                raise NotFeasiblePoints("[ERROR] No feasible points were found in the constraint space! # tries: %d." %
                                        MFDGPHandler.MAX_TRIES_FOR_FEASIBLE_GRID)
        pareto_set, pareto_front, self.samples_objs, self.samples_cons = res
        self.set_pareto_solution(pareto_set, pareto_front)
        return self.pareto_set, self.pareto_front, self.samples_objs, self.samples_cons

    def _moop_search_kwargs(self):
        return {"search": self.pareto_search, "evolve_population": self.pareto_evolve_population,
                "evolve_generations": self.pareto_evolve_generations}

    def sample_and_store_pareto_solution(self, seed=None, **kw):
        """Pareto solution of one posterior sample of the problem, stored for the conditioned training.

        Single process, ``seed=None``: the reference's procedure on this process's generators (``nFeatures``, ``generator``,
        ``rng`` pass through).  With a process group (black-boxes sharded over ranks) or a ``seed``: the seeded joint
        procedure of ``_sample_and_store_pareto_solution_seeded``, identical on every rank and independent of the sharding;
        with a group and no seed, rank 0 draws the seed from torch's global generator and broadcasts it."""
        from .moop import NotFeasiblePoints
        if self.pareto_search == "evolve" and not parallel._no_group():
            raise ValueError("pareto_search='evolve' is limited to one process (surrogates sharded over a process group take "
                             "pareto_search='grid')")
        seeded = seed is not None or not parallel._no_group()
        if seeded:
            unknown = set(kw) - {"nFeatures"}
            if unknown:
                raise TypeError("seeded Pareto sampling takes nFeatures only (got %s)" % sorted(unknown))
            if seed is None:
                dev = parallel._exchange_device()
                t = torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).to(dev)
                seed = int(parallel.broadcast_(t, 0).cpu()[0])
        attempt = 0
        while True:
            try:
                if seeded:
                    return self._sample_and_store_pareto_solution_seeded(seed, attempt=attempt, **kw)
                return self._sample_and_store_pareto_solution(**kw)
            except NotFeasiblePoints:
                print("Not feasible solution found, trying another time!")
                sys.stdout.flush()
                attempt += 1

    @staticmethod
    def _pareto_sample_seed(seed, k):
        """The seed of Pareto sample k of ``conditioned_copies``: ``seed`` itself for k = 0 (one sample is the plain seeded
        call), else a 62-bit function of (seed, k) alone, in the style of ``_blackbox_generator``."""
        if seed is None or k == 0:
            return seed
        import hashlib
        key = hashlib.sha256(("%d:PARETO_SAMPLE:%d" % (int(seed), int(k))).encode()).digest()
        return int.from_bytes(key[:8], "big") >> 2

    def conditioned_copies(self, K, seed=None, **sample_kw):
        """K fitters conditioned on K sampled Pareto sets (JESMOC_MFDGP(num_pareto_samples=K)): ``[self, copy_1 ...
        copy_{K-1}]``.  The copies are ``copy_uncond()`` of this fitter taken BEFORE it is conditioned; then, one after the other
        (never concurrently: the one-launch conditioned steps wait inside the launch and assume an otherwise idle device), every
        fitter samples its Pareto solution and trains its conditioned surrogates.  This fitter keeps a solution it already holds.
        ``seed=None``: the unseeded procedure on the process generators, in order; else sample k is the seeded procedure with
        ``_pareto_sample_seed(seed, k)``.  ``sample_kw`` pass to ``sample_and_store_pareto_solution``."""
        K = int(K)
        if K < 1:
            raise ValueError("conditioned_copies: K >= 1 (got %d)" % K)
        if K > 1 and not parallel._no_group():
            raise ValueError("conditioned_copies: several Pareto samples (K = %d) are limited to one process; surrogates "
                             "sharded over a process group take K = 1" % K)
        fitters = [self] + [self.copy_uncond() for _ in range(K - 1)]
        for k, fitter in enumerate(fitters):
            if k > 0 or getattr(fitter, "pareto_set", None) is None:
                fitter.sample_and_store_pareto_solution(seed=self._pareto_sample_seed(seed, k), **sample_kw)
            fitter.train_conditioned_mfdgps()
        return fitters

    # status words of one try of the seeded procedure (rank 0's decides; ERROR anywhere makes every rank raise)
    _FEASIBLE, _INFEASIBLE, _ERROR = 0, 1, 2

    @staticmethod
    def _blackbox_generator(seed, role, gi, t):
        """The generator of black-box (role, global index gi)'s sample in try t: a function of these four numbers only, so
        the draws do not depend on the rank, the world size or the order the black-boxes are visited in."""
        import hashlib
        key = hashlib.sha256(("%d:%s:%d:%d" % (int(seed), role, int(gi), int(t))).encode()).digest()
        return torch.Generator().manual_seed(int.from_bytes(key[:8], "big") >> 1)

    def _draw_chain_samples(self, seed, t, nFeatures):
        """This rank's chain samples of try t: (packed buffers, global indices, roles 0 = objective / 1 = constraint)."""
        from ..layers.rff import sample_chain_from_posterior
        bufs, idx, roles = [], [], []
        for tag, i, h in self._handlers():
            gi = self._global_index(h, i)
            smp = sample_chain_from_posterior(h.mfdgp, nFeatures=nFeatures,
                                              generator=self._blackbox_generator(seed, tag, gi, t))
            bufs.append(smp.pack())
            idx.append(gi)
            roles.append(0 if tag == "OBJ" else 1)
        return bufs, idx, roles

    def _agree(self, code, res, n_obj, d):
        """One status word per rank, all-gathered; rank 0's result broadcast (row count first, then set and front in one
        buffer).  Every rank makes the same collective calls whatever happened locally."""
        dev = parallel._exchange_device() if not parallel._no_group() else torch.device("cpu")
        P = int(res[0].shape[0]) if (code == self._FEASIBLE and res is not None) else 0
        status = torch.cat(parallel.all_gather_ragged(torch.tensor([[float(code), float(P)]], dtype=torch.float64,
                                                                   device=dev)), 0).cpu()
        errs = [q for q in range(status.shape[0]) if int(status[q, 0]) == self._ERROR]
        if errs:
            return self._ERROR, errs
        code0, P0 = int(status[0, 0]), int(status[0, 1])
        if code0 != self._FEASIBLE:
            return code0, None
        buf = torch.zeros(P0, d + n_obj, dtype=torch.float64, device=dev)
        if parallel.world()[0] == 0:
            buf.copy_(torch.cat([res[0], res[1]], 1).to(dev))
        parallel.broadcast_(buf, 0)
        buf = buf.cpu()
        return code0, (buf[:, :d].clone(), buf[:, d:].clone())

    def _sample_and_store_pareto_solution_seeded(self, seed, nFeatures=500, attempt=0):
        """The Pareto solution of one joint posterior sample of ALL black-boxes, whichever rank holds them.

        Try t draws every local black-box's chain sample from ``_blackbox_generator(seed, role, global index, t)``, all ranks
        exchange the packed samples (``parallel.all_gather_samples``, which also checks that every rank has the same
        training inputs) and unpack all of them -- their own too, so every rank holds identical objects -- then run the same
        MOOP on the grid of ``np.random.default_rng((seed, t))``.  Rank 0's outcome decides (feasible / next try / after
        MAX_TRIES_FOR_FEASIBLE_GRID tries the least infeasible points / NotFeasiblePoints) and its set and front are
        broadcast, so every rank stores bitwise the same solution.  An exception on any rank after the exchange makes every
        rank raise.  ``samples_objs`` / ``samples_cons`` hold all black-boxes' samples in global order.  Without a process
        group every exchange is the identity and the result is the same as with the black-boxes split over ranks.
        ``attempt`` (the retries after NotFeasiblePoints) moves the tries to fresh numbers."""
        import hashlib
        from ..layers.rff import RFFChainSample
        from .moop import MOOP, NotFeasiblePoints
        inputs = np.ascontiguousarray(self.x_train.detach().cpu().double().numpy())
        d = inputs.shape[1]
        xhash = float(int.from_bytes(hashlib.sha256(inputs.tobytes() + str(inputs.shape).encode()).digest()[:6], "big"))
        thr_src = self.thresholds_cons_global if self.thresholds_cons_global is not None else self.thresholds_cons
        feasible = -1.0 * thr_src.detach().cpu().double().numpy()
        dev = torch.device(self.device)
        sample_dev = dev if dev.type == "cuda" else None
        tries = MFDGPHandler.MAX_TRIES_FOR_FEASIBLE_GRID
        t0 = attempt * tries
        optimizer, objs, cons = None, None, None
        for t in range(t0, t0 + tries + 1):
            fallback = t == t0 + tries          # the least infeasible points of the last try's samples
            if not fallback:
                err = None
                try:
                    bufs, idx, roles = self._draw_chain_samples(seed, t, nFeatures)
                except Exception as e:          # said inside the exchange: the peers must not wait in it
                    err, bufs, idx, roles = e, [], [], []
                allo, allc = parallel.all_gather_samples(bufs, idx, roles=roles, check=xhash, local_error=err)
            code, res, local_exc = self._ERROR, None, None
            try:
                if not fallback:
                    objs = [RFFChainSample.unpack(b, sample_dev) for b in allo]
                    cons = [RFFChainSample.unpack(b, sample_dev) for b in allc]
                    if len(cons) != feasible.shape[0]:
                        raise ValueError("%d constraint samples but %d thresholds (sharded black-boxes need "
                                         "set_global_constraint_thresholds)" % (len(cons), feasible.shape[0]))
                    optimizer = MOOP(objs, cons, input_dim=d, grid_size=self.opt_grid_size * d,
                                     pareto_set_size=self.pareto_set_size, feasible_values=feasible,
                                     rng=np.random.default_rng((int(seed), int(t))), refine=self.pareto_refine,
                                     **self._moop_search_kwargs())
                    res = optimizer.compute_pareto_solution_from_samples(inputs)
                else:
                    res = optimizer.compute_pareto_solution_from_samples(inputs, allow_negative_constraints=True)
                code = self._FEASIBLE if res is not None else self._INFEASIBLE
            except Exception as e:
                local_exc = e
            code, out = self._agree(code, res, len(objs) if objs is not None else 0, d)
            if code == self._ERROR:
                msg = "Pareto sampling failed on rank(s) %s" % out
                if local_exc is not None:
                    raise RuntimeError(msg + ": " + repr(local_exc)) from local_exc
                raise RuntimeError(msg)
            if code == self._FEASIBLE:
                break
        else:
            raise NotFeasiblePoints("[ERROR] No feasible points were found in the constraint space! # tries: %d." % tries)
        self.samples_objs, self.samples_cons = objs, cons
        self.set_pareto_solution(*out)
        return self.pareto_set, self.pareto_front, self.samples_objs, self.samples_cons

    # ------------------------------------------------------------------ conditioned training
    def set_pareto_solution(self, pareto_set, pareto_front):
        """Pareto set (P, d) / front (P, n_obj) to condition on: from ``sample_and_store_pareto_solution`` (the
        reference's route, :181-225) or from any other optimiser."""
        dev = torch.device(self.device)
        self.pareto_set = pareto_set.double().to(dev)
        self.pareto_front = pareto_front.double().to(dev)

    def _thresholds_on(self, device, all_constraints=False):
        """Device copy of the constraint thresholds (uploaded once: a host->device copy is not capturable).
        ``all_constraints``: the vector over the constraints of every rank (omega factors), else this rank's own."""
        src = self.thresholds_cons_global if (all_constraints and self.thresholds_cons_global is not None) \
            else self.thresholds_cons
        c = getattr(self, "_thr_cache", None) or {}
        hit = c.get(all_constraints)
        if hit is None or hit[0] is not src or hit[1].device != torch.device(device):
            hit = (src, src.to(device))
            c[all_constraints] = hit
            self._thr_cache = c
        return hit[1]

    @staticmethod
    def _global_index(h, local_index):
        return local_index if getattr(h, "global_index", None) is None else h.global_index

    def loss_theta_factors(self, cs_mean, cs_var, threshold):
        """:227-233.  On the GPU one launch (functional.cond_factors); host tensors: the plain torch statement."""
        if cs_mean.is_cuda:
            thr = threshold.reshape(1) if torch.is_tensor(threshold) else torch.tensor([float(threshold)], dtype=cs_mean.dtype,
                                                                                     device=cs_mean.device)
            return F.cond_factors([], [], [cs_mean.reshape(-1)], [cs_var.reshape(-1)], None, thr,
                                  float(np.log(1.0 - self.eps)), float(np.log(self.eps)))
        c = _ncdf((cs_mean - threshold) / torch.sqrt(cs_var))
        return torch.sum(np.log(1.0 - self.eps) * c + np.log(self.eps) * (1.0 - c))

    def loss_omega_factors(self, fs_mean, fs_var, cs_mean, cs_var, pareto_front):
        """:235-243.  fs_* (n_obj, T), cs_* (n_con, T) -- stacked tensors or lists of rows.  On the GPU one launch
        (functional.cond_factors: forward, gradients included); host tensors: the plain torch statement."""
        rows = lambda t: list(t) if isinstance(t, (list, tuple)) else list(t.unbind(0))
        fm, fv, cm, cv = rows(fs_mean), rows(fs_var), rows(cs_mean), rows(cs_var)
        ref = fm[0] if fm else cm[0]
        thr = self._thresholds_on(ref.device, all_constraints=True)
        if thr.numel() != len(cm):
            raise ValueError("omega factors: %d constraint rows but %d thresholds (sharded surrogates need "
                             "set_global_constraint_thresholds)" % (len(cm), thr.numel()))
        if ref.is_cuda and len(fm) <= 8 and len(cm) <= 8:
            front = self._cached_const(("front", id(pareto_front)), lambda: pareto_front.contiguous())
            return F.cond_factors(fm, fv, cm, cv, front, thr, float(np.log(self.eps)), float(np.log(1.0 - self.eps)))
        fs_mean, fs_var = torch.stack(fm), torch.stack(fv)
        c = torch.ones(fs_mean.shape[-1], dtype=fs_mean.dtype, device=fs_mean.device)
        if cm:
            cs_mean, cs_var = torch.stack(cm), torch.stack(cv)
            c = _prod(_ncdf((cs_mean - thr[:, None]) / torch.sqrt(cs_var)), 0)
        c = c * _prod(_ncdf((pareto_front[:, :, None] - fs_mean) / torch.sqrt(fs_var)), 1)
        return torch.sum(np.log(self.eps) * c + np.log(1 - self.eps) * (1.0 - c))

    def next_conditioned_batch(self, h):
        """The training batch of one model for one conditioned iteration (:281-285, :296-300): the whole data set when the
        handler trains full-batch (every example of the reference: batch_size = N; the loss does not depend on the row
        order), otherwise the next batch of the model's own shuffling loader, re-armed when it runs out."""
        if h.batch_size >= h.num_data:
            return h.train_dataset.tensors
        try:
            return next(h.iter_train_loader)
        except (TypeError, StopIteration):
            h.iter_train_loader = iter(h.train_loader)
            return next(h.iter_train_loader)

    def conditioned_loss(self, x_tilde, eps=None, batches=None):
        """The joint loss of one conditioned-training iteration (:270-343).  ``batches``: optional {(tag, i): (x, y, fid)}
        replacing the loader draw (tests).

        The reference runs three forwards per model (training batch, Pareto set, x_tilde); the layer is separable over
        rows, so here they are ONE forward on the concatenated rows: one Cholesky chain and one set of GEMMs per layer
        instead of three.  ``eps``: optional {name: [None, eps_l1, ...]} with draws for the concatenated rows.
        With surrogates sharded over ranks the omega factors need every model's (mean, var) at x_tilde: the local ones
        carry gradient, the others arrive as constants through one all-gather (mobocmf_amd.parallel)."""
        P, T = self.pareto_set.shape[0], x_tilde.shape[0]
        # The loss is a signed sum of scalar terms.  They are collected and combined in ONE launch at the end, the rows of every
        # layer's moments are split into their three ranges (training batch | Pareto set | x~) by one autograd node per layer,
        # and the theta / omega factors are one launch each: as framework ops (a subtraction per term, slice / stack backward
        # per range, cdf / product / sum chains) this glue was ~100 element-wise launches per iteration of a loop whose cost IS
        # its launch count.
        terms, coefs = [], []
        tilde = {}
        k = 0
        log_e, log_1me = float(np.log(self.eps)), float(np.log(1.0 - self.eps))
        for tag, i, h in self._handlers():
            xb, yb, fb = batches[(tag, i)] if batches is not None else self.next_conditioned_batch(h)
            B = xb.shape[0]
            S = h.mfdgp.num_samples_for_training
            top = h.num_fidelities - 1
            out = h.mfdgp(torch.cat([xb, self.pareto_set, x_tilde], 0), eps=None if eps is None else eps[(tag, i)])
            parts = []
            for d in out:
                rpb = d.mean.numel() // (B + P + T)      # rows of the layer per input row
                parts.append(F.split_rows(d.mean, d.variance, [B * rpb, P * rpb, T * rpb]))
            batch = [MVN(pm[0], pv[0]) for pm, pv in parts]
            terms.append(h.elbo(batch, yb.T, fb)[0])
            coefs.append(-float(h.num_data) / B)
            mu_p, var_p = parts[top][0][1], parts[top][1][1]
            if tag == "OBJ":
                pf = self._cached_const(("pf", top, P), lambda: torch.full((P, 1), float(top), dtype=xb.dtype, device=xb.device))
                pl = [None] * top + [MVN(mu_p, var_p)]
                gi = self._global_index(h, i)                 # the front's columns follow the GLOBAL objective order
                col = self._cached_const(("front_col", gi), lambda: self.pareto_front[:, gi:gi + 1].T.contiguous())
                terms.append(h.elbo(pl, col, pf, include_kl_term=False))
                coefs.append(-1.0)
            else:
                if S > 1:
                    raise NotImplementedError("theta factors are defined for one sample per row (reference: S = 1)")
                thr_k = self._thresholds_on(xb.device)[k:k + 1]
                terms.append(F.cond_factors([], [], [mu_p], [var_p], None, thr_k, log_1me, log_e))      # :227-233
                coefs.append(-1.0)
                k += 1
            tilde[(tag, i)] = (parts[top][0][2], parts[top][1][2])
        fm = [tilde[(t, i)][0] for t, i, _ in self._handlers() if t == "OBJ"]
        fv = [tilde[(t, i)][1] for t, i, _ in self._handlers() if t == "OBJ"]
        cm = [tilde[(t, i)][0] for t, i, _ in self._handlers() if t == "CON"]
        cv = [tilde[(t, i)][1] for t, i, _ in self._handlers() if t == "CON"]
        if parallel.world()[1] > 1:
            oi = [self._global_index(h, i) for t, i, h in self._handlers() if t == "OBJ"]
            ci = [self._global_index(h, i) for t, i, h in self._handlers() if t == "CON"]
            stk = lambda rows: torch.stack(rows) if rows else x_tilde.new_zeros((0, T))
            gfm, gfv, gcm, gcv = parallel.gather_with_local_grad(stk(fm), stk(fv), stk(cm), stk(cv), oi, ci)
            fm, fv, cm, cv = list(gfm.unbind(0)), list(gfv.unbind(0)), list(gcm.unbind(0)), list(gcv.unbind(0))
        terms.append(self.loss_omega_factors(fm, fv, cm, cv, self.pareto_front))
        coefs.append(-1.0)
        return F.scalar_combine(terms, coefs)

    def _cached_const(self, key, make):
        """Small constant device tensors of the conditioned loss, built once (a fill / copy launch per iteration otherwise)."""
        c = self.__dict__.setdefault("_const_cache", {})
        hit = c.get(key)
        if hit is None or hit[0] is not self.pareto_front:
            hit = (self.pareto_front, make())
            c[key] = hit
        return hit[1]

    def train_conditioned_mfdgps(self, num_iters=None, use_graphs=None):
        """ONE Adam over all models' parameters, kernel hyper-parameters frozen (:245-268, :345-354).  On the GPU the
        whole iteration (x~ draw, joint loss over all surrogates, backward, Adam) is replayed from a HIP graph; a failed
        Cholesky inside a replay rolls back to the last verified state and continues eagerly (jitter ladder)."""
        for _, _, h in self._handlers():
            h.mfdgp.fix_variational_hypers_cond(True)
        num_iters = self.num_epochs_2 if num_iters is None else num_iters
        full_batch = all(h.batch_size >= h.num_data for _, _, h in self._handlers())
        if use_graphs is None:
            use_graphs = self.pareto_set.is_cuda and parallel.world()[1] == 1 and full_batch
        if use_graphs and not full_batch:
            raise ValueError("a captured conditioned step needs batch_size >= number of training points (mini-batches come "
                             "from a host-side loader)")
        if self._natgrad() and not full_batch:
            raise ValueError("variational_optimizer='natgrad' needs batch_size >= number of training points in the conditioned "
                             "fit (mini-batches come from a host-side loader)")
        tiny = None
        if use_graphs and self.use_tiny_step and parallel.world()[1] == 1 and self._one_launch_allowed():
            # the reference's own sizes: the whole iteration in 3 + n_con launches (util/tiny_step.py)
            done, tiny = self._train_conditioned_tiny(num_iters)
            num_iters -= done
        if num_iters > 0:
            step = graphed_step.GraphedConditionedStep(self, lr=self.lr_2, use_graph=use_graphs,
                                                       stream=self._stream_for(0, self.pareto_set.device)
                                                       if self.pareto_set.is_cuda else None, **self._optimizer_kwargs())
            if tiny is not None:      # a Cholesky failed there: this path (jitter ladder) continues with its optimiser state
                for k in range(len(tiny.models)):
                    tiny.export_adam_state(k, step.optimizer)
            run_verified([step], num_iters, REDO_EAGERLY, ["conditioned training: "], "iterations",
                         self._report_iter(num_iters))
        for _, _, h in self._handlers():
            h.iter_train_loader = None
            h.mfdgp.set_check_pd(True)

    def _train_conditioned_tiny(self, num_iters):
        """Conditioned training through TinyConditionedStep when every surrogate fits it.  Returns (iterations completed, step
        or None): fewer than ``num_iters`` when the surrogates do not fit (0, None) or after a failed Cholesky (state rolled
        back to the last verified iteration; the layer path continues)."""
        dev = self.pareto_set.device
        step = None
        # M <= 32 in one workgroup per surrogate, M <= 128 in several
        for cls in (tiny_step.TinyConditionedStep, coop_step.CoopConditionedStep):
            try:
                step = cls(self, lr=self.lr_2, stream=self._stream_for(0, dev), **self._optimizer_kwargs())
                break
            except _lib.MobocmfError:
                continue
        if step is None:
            return 0, None
        step.stream.wait_stream(torch.cuda.current_stream(dev))
        return run_verified([step], num_iters, HAND_OVER, ["conditioned training: "], "iterations",
                            self._report_iter(num_iters))[0], step

    def _report_iter(self, num_iters):
        """run_verified's ``report`` of the conditioned drivers (None when not verbose)."""
        def report(i, _, step):
            print("Iter:", i, "/", num_iters, ". Neg. ELBO per iter:", step.loss.item())
            sys.stdout.flush()
        return report if self.verbose else None

    # ------------------------------------------------------------------ recommendation (the reference's BO driver)
    def recommend(self, grid, min_feasible_prob=0.999, output_scaling=None, search="grid", evolve_population=128,
                  evolve_generations=100, evolve_seed=0):
        """The recommended Pareto set of the BO loop.  ``search="grid"``: the rule of ``_recommend_grid`` on the rows of ``grid``.
        ``search="evolve"``: the grid stage first; then NSGA-II on the GPU over the same predictions under the same feasibility
        rule (util/recommend_evolve.py, a generation per graph replay) from a population of ``evolve_population`` grid rows --
        the grid's front, thinned to half the population by ``MOOP.compute_pareto_front_and_set_summary_y_space`` when it has
        more rows, then the other rows by (violation ascending, row index); the largest even count; with fewer than 4 rows no
        evolution -- for ``evolve_generations`` generations with the Philox key ``evolve_seed``.  The final rows the device calls
        feasible that lie farther than 1e-6 from every grid row are appended to the grid and the grid stage decides over the
        union: the returned set obeys exactly the grid mode's rule, and every row of the grid's front is in it or dominated by
        one of its rows.  One process only; surrogates no predict group takes raise ValueError (there is no host fallback).

        Returns (pareto_set, predicted_front, info) as ``_recommend_grid``; with "evolve" the kept grid rows come first, in row
        order, then the kept evolved rows; ``info["mask"]`` stays the mask over the grid's rows, the counts are those of the
        union, and ``info`` gains ``population`` (Np, d) the final population, ``evolved_mask`` (Np,) its rows in the returned
        set, ``num_evolved``, ``generations`` and ``engine`` (the predict group's class name; None without evolution)."""
        if search not in ("grid", "evolve"):
            raise ValueError("search must be 'grid' or 'evolve' (got %r)" % (search,))
        if not 4 <= int(evolve_population) <= 512 or int(evolve_population) % 2:
            raise ValueError("evolve_population must be even, 4..512 (got %r)" % (evolve_population,))
        if int(evolve_generations) < 1:
            raise ValueError("evolve_generations must be >= 1")
        if search == "grid":
            return self._recommend_grid(grid, min_feasible_prob, output_scaling)
        if parallel.world()[1] != 1:
            raise ValueError("recommend: search='evolve' runs in one process only")
        return self._recommend_evolve(grid, min_feasible_prob, output_scaling, int(evolve_population), int(evolve_generations),
                                      int(evolve_seed))

    def _recommend_evolve(self, grid, p_min, output_scaling, Np, generations, seed):
        from .moop import MOOP
        from .recommend_evolve import RecommendEvolve
        _, grid_front, info = self._recommend_grid(grid, p_min, output_scaling)
        grid_np = np.ascontiguousarray(grid.detach().cpu().numpy() if torch.is_tensor(grid) else np.asarray(grid),
                                       dtype=np.float64)
        n, d = grid_np.shape
        pop = min(Np, n) // 2 * 2
        new, X, generations_run, engine = np.zeros(0, dtype=np.int64), np.zeros((0, d)), 0, None
        if pop >= 4:
            # objectives, then constraints, each in global-index order: the order of the grid stage
            hs = sorted(self._handlers(), key=lambda e: (e[0] != "OBJ", self._global_index(e[2], e[1])))
            names = {id(h): name for name, h in list(self.mfdgp_handlers_objs.items()) + list(self.mfdgp_handlers_cons.items())}
            scale = None
            if output_scaling is not None:
                scale = [[float(output_scaling[names[id(h)]][0]), float(output_scaling[names[id(h)]][1])] for _, _, h in hs]
            eng = RecommendEvolve([h.mfdgp for _, _, h in hs], self.num_obj, self.num_fidelities - 1, pop, d, seed, p_min=p_min,
                                  scale=scale)
            try:
                _, viol = eng.score(grid_np)
                viol = viol.cpu().numpy()
                front = np.flatnonzero(info["mask"])
                if front.size > pop // 2:
                    front = MOOP.compute_pareto_front_and_set_summary_y_space(None, front[:, None], grid_front, pop // 2)[0][:, 0]
                rest = np.setdiff1d(np.arange(n), front)
                rest = rest[np.lexsort((rest, viol[rest]))][:pop - front.size]
                eng.start(torch.from_numpy(grid_np[np.concatenate((front, rest))]))
                eng.run(generations)
                out = eng.result()
                X, Fv, ev = (out[key].cpu().numpy() for key in ("X", "F", "viol"))
            except BaseException:      # (the group must not keep chains of parameters that may change)
                eng.group.thaw()
                raise
            eng.finish()
            new = np.array([i for i in np.flatnonzero(ev == 0.0)
                            if not np.isnan(Fv[:, i]).any() and np.min(np.sqrt(((grid_np - X[i]) ** 2).sum(1))) > 1e-6],
                           dtype=np.int64)
            generations_run, engine = generations, type(eng.group).__name__
        evolved_mask = np.zeros(X.shape[0], dtype=bool)
        if new.size:
            union = np.vstack((grid_np, X[new]))
            pareto_set, front_vals, info = self._recommend_grid(union, p_min, output_scaling)
            evolved_mask[new] = info["mask"][n:]
            info = dict(info, mask=info["mask"][:n])
        else:
            pareto_set = grid_np[info["mask"]]
            front_vals = grid_front
        info.update(population=X, evolved_mask=evolved_mask, num_evolved=int(evolved_mask.sum()), generations=generations_run,
                    engine=engine)
        return pareto_set, front_vals, info

    def _recommend_grid(self, grid, min_feasible_prob=0.999, output_scaling=None):
        """The recommended Pareto set of the reference's BO loop (toy_synthetic_2D_JESMOCMF.py:537-573): every black-box's
        top-fidelity ``predict_for_acquisition`` moments on ``grid`` (n, d), the top layer's likelihood noise subtracted from
        the constraint variances, optionally un-standardised (``output_scaling``: black-box name -> (mean, std); means
        m std + mean, variances and noise times std^2), then ONE ``functional.pareto_mask``: the grid rows where every
        constraint has Phi(m / sqrt(v - noise)) > ``min_feasible_prob`` and whose predicted objective means are
        non-dominated among those rows.

        With the black-boxes sharded over ranks every rank gathers the moment rows of all of them
        (``parallel.all_gather_ragged``), orders them by role and global index and computes the same mask: every rank returns
        the same result.  Returns (pareto_set (P, d) ndarray, predicted_front (P, n_obj) ndarray, info dict with the grid
        mask and the counts of feasible, front and NaN rows).  Raises when a feasible row has a NaN predicted objective,
        and on every rank when any rank failed to predict."""
        _lib.require_device()
        dev = torch.device(self.device)
        if dev.type != "cuda":
            raise _lib.MobocmfError("recommend: the fitter's models must live on the GPU (device=%r)" % self.device)
        grid_np = np.ascontiguousarray(grid.detach().cpu().numpy() if torch.is_tensor(grid) else np.asarray(grid),
                                       dtype=np.float64)
        if grid_np.ndim != 2:
            raise _lib.MobocmfError("recommend: grid must be (n, d)")
        n = grid_np.shape[0]
        top = self.num_fidelities - 1
        names = {id(h): name for name, h in list(self.mfdgp_handlers_objs.items()) + list(self.mfdgp_handlers_cons.items())}
        rows, err = [], None
        try:
            x = torch.from_numpy(grid_np).to(dev)
            with torch.no_grad():
                for tag, i, h in self._handlers():
                    mean, var = h.mfdgp.predict_for_acquisition(x, top)
                    mean, var = mean.reshape(-1), var.reshape(-1)
                    noise = getattr(h.mfdgp, h.mfdgp.name_hidden_layer_likelihood + str(top)).noise.reshape(-1)[0]
                    noise = noise.to(dev, torch.float64)
                    if output_scaling is not None:
                        mu, sd = output_scaling[names[id(h)]]
                        mean, var, noise = mean * float(sd) + float(mu), var * float(sd) ** 2, noise * float(sd) ** 2
                    head = torch.tensor([0.0 if tag == "OBJ" else 1.0, float(self._global_index(h, i))], dtype=torch.float64,
                                        device=dev)
                    rows.append(torch.cat([head, noise.reshape(1), mean, var]))
            local = torch.stack(rows) if rows else torch.zeros(0, 3 + 2 * n, dtype=torch.float64, device=dev)
        except Exception as e:                   # said inside the exchange: the peers must not wait in it
            err = e
            local = torch.full((1, 3 + 2 * n), -1.0, dtype=torch.float64, device=dev)
        allr = torch.cat(parallel.all_gather_ragged(local), 0).to(dev)
        if err is not None:
            raise RuntimeError("recommend: prediction failed on this rank: %r" % err) from err
        if bool((allr[:, 0] < 0).any()):
            raise RuntimeError("recommend: prediction failed on another rank")
        head = allr[:, :2].cpu().numpy()
        order = np.lexsort((head[:, 1], head[:, 0]))          # objectives, then constraints, each in global order
        allr = allr[torch.from_numpy(order).to(dev)]
        role, gi = head[order, 0], head[order, 1]
        for r in (0.0, 1.0):
            idx = gi[role == r]
            if not np.array_equal(idx, np.arange(idx.size)):
                raise RuntimeError("recommend: the %s global indices over all ranks are %s, not 0..%d"
                                   % ("objective" if r == 0 else "constraint", idx.tolist(), idx.size - 1))
        obj, con = allr[role == 0.0], allr[role == 1.0]
        if obj.shape[0] == 0:
            raise _lib.MobocmfError("recommend: no objective")
        vals = obj[:, 3:3 + n]
        if con.shape[0]:
            mask, counts = F.pareto_mask(vals, con[:, 3:3 + n], con[:, 3 + n:], con[:, 2], p_min=min_feasible_prob)
        else:
            mask, counts = F.pareto_mask(vals, p_min=min_feasible_prob)
        counts = counts.cpu().tolist()
        if counts[2]:
            raise _lib.MobocmfError("recommend: %d probably-feasible grid rows have a NaN predicted objective" % counts[2])
        mask_np = mask.cpu().numpy()
        front = vals.T[mask].cpu().numpy()
        info = {"mask": mask_np, "num_feasible": counts[0], "num_front": counts[1], "num_nan": counts[2]}
        return grid_np[mask_np], front, info

    def mfdgps_to_train_mode(self):
        for _, _, h in self._handlers():
            h.mfdgp.train()

    def mfdgps_to_eval_mode(self):
        for h in self.mfdgp_handlers_objs.values():
            h.mfdgp.eval()
        for h in self.mfdgp_handlers_cons.values():
            h.mfdgp.train()                      # as written in the reference (:363-368)

    def copy_uncond(self):
        """Deep copy of the fitter (:372-397): the models only hold tensors, so ``deepcopy`` just works."""
        for _, _, h in self._handlers():
            h.mfdgp.eval()
        self_copy = deepcopy(self)
        for _, _, h in self._handlers() + self_copy._handlers():
            h.mfdgp.train()
        return self_copy
