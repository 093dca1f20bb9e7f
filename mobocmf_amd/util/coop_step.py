"""The ELBO step of MID-SIZE surrogates (M <= 128 inducing points) as ONE launch for a whole group of models, several
workgroups per surrogate: mobocmf_coop_elbo_step (csrc/coop_step.hip).

The reference's own BO loop trains M = N from 15 to 75 points (examples/toy_synthetic_2D_JESMOCMF/...py:25,102-103,305-331 with
mfdgp.py:295-298); the one-workgroup kernel (util/tiny_step.py) covers M <= 32, the layer path costs 57 launches per step there.
``CoopELBOStep`` has the surface of ``TinyELBOStep`` / ``GraphedELBOStep`` that the fitter's loop uses (step / check / snapshot /
restore / losses / export_adam_state); ``CoopConditionedStep`` is the conditioned iteration (blackbox_mfdgp_fitter.py:245-354).
"""
from .. import _lib
from . import tiny_step as TS

MAX_COLUMNS = 16384              # rows[l] * S per layer this binding accepts
MAX_PREDICT_COLUMNS = 4096       # T * S per layer beyond which the layer path (frozen chains) is the better search engine
MAX_WORTHWHILE_COLUMNS = 2048    # summed over the layers: beyond, the layer path's grid-filling launches win (tools/coop_sweep.py)

# several workgroups per surrogate (csrc/coop_step.hip); a coupled launch takes as many models as the device keeps resident
COOP = TS.Kernel("mobocmf_coop_elbo_step", "mobocmf_coop_work_bytes", _lib.COOP_MAX_M, MAX_COLUMNS, MAX_PREDICT_COLUMNS, None,
                 cooperative=True)


def eligible(model, x, fidelities):
    """The structural limits of the cooperative kernel: <= 3 layers sharing one set of <= 128 inducing inputs, d <= 8, softplus /
    Interval constraints, float64 parameters on the GPU (``tiny_step.eligible`` with this kernel's limits; no speed rule: the
    launch beats the layer path's ~57 launches per step wherever it applies)."""
    return TS.eligible(model, x, fidelities, speed_rule=False, kernel=COOP)


def worthwhile(model, x, fidelities):
    """``eligible`` and small enough for the launch to beat the layer path (profiles/r05_coop_step.txt: BASELINE config 2 --
    M = 128, 512 + 1024 columns -- 1.3x; the reference's loop sizes 2-2.5x; a single workgroup round per phase is what wins, so
    the gate is the number of columns)."""
    if not eligible(model, x, fidelities):
        return False
    S = model.num_samples_for_training
    rows = TS.rows_per_layer(fidelities, len(model._layers()))
    return sum(r * (S if l else 1) for l, r in enumerate(rows)) <= MAX_WORTHWHILE_COLUMNS


def fits_predict(model, fidelity, T, d):
    """``tiny_step.fits_predict`` with the cooperative kernel's limits (M <= 128) and its column bound."""
    return TS.fits_predict(model, fidelity, T, d, speed_rule=False, kernel=COOP)


class CoopELBOStep(TS.TinyELBOStep):
    """``step()`` == one full-batch ELBO step of EVERY model of the group, one launch (see ``TinyELBOStep`` for the arguments)."""
    kernel = COOP


class CoopConditionedStep(TS.TinyConditionedStep):
    """One iteration of the conditioned training in ONE launch (STEP_COUPLED), or forward-only launch + factor launches + step
    launch."""
    kernel = COOP


class CoopPredictGroup(TS.TinyPredictGroup):
    """``TinyPredictGroup`` for mid-size models (32 < M <= 128): predictive moments of several fitted models at the same T test
    points in ONE cooperative launch (STEP_FORWARD), their gradient w.r.t. the test points in one more (STEP_INPUT_GRADIENTS) --
    the acquisition search of the reference's later BO iterations (JESMOC_MFDGP.py:137-184 against M = N = 33 ... 75
    surrogates).  A give-up of an in-launch wait is reported by ``thaw()``, at the end of the search.  (``why_not``: inherited,
    with this class's ``kernel``: ``fits_predict`` above.)"""
    kernel = COOP
    _frozen = False            # inside freeze() ... thaw(): the models' parameters do not change between launches
    _chain_ready = False       # ... and a launch since freeze() has left their chains (L^-1, U, a) in the workspaces

    def freeze(self):
        """The parameters are constants until ``thaw()`` (an acquisition search, JESMOC_MFDGP._optimize): the first launch
        computes the chains, the following ones reuse them (MOBOCMF_STEP_CHAIN_VALID)."""
        if not self._frozen:
            self._frozen, self._chain_ready = True, False

    def thaw(self):
        """Ends the search; synchronising: raises InLaunchWaitAbandoned if a launch since the last thaw() gave up a wait (its
        moments were invalid; the words are cleared, the next search starts afresh)."""
        self._frozen = self._chain_ready = False
        sync = self.__dict__.get("sync")
        if sync is not None:
            sync.check("cooperative predict group")

    def _launch(self, mode):
        if self._frozen and self._chain_ready:
            mode |= _lib.STEP_CHAIN_VALID
        super()._launch(mode)
        self._chain_ready = self._frozen
