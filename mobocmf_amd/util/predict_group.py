"""What the predict groups -- TinyPredictGroup (util/tiny_step.py), CoopPredictGroup (util/coop_step.py), PanelPredictGroup and
SplitPredictGroup (util/panel_predict.py) -- share and an acquisition search drives (JESMOC_MFDGP, util/acq_search.py).  A group
has ``models``, ``device``, ``stream``, ``fidelity``, ``T``, ``d``, ``S``, the buffers ``x`` (T, d), ``moments`` (n, 2, T S), ``seeds``
(like moments) and ``gx`` (n, T, d), ``info_words`` and ``_launch(mode)``."""
import contextlib

import torch

from .. import _lib


class _MomentsFn(torch.autograd.Function):
    """(n_models, 2, columns) top-layer moments of a predict group at X; backward: d / d X through every model, one launch."""

    @staticmethod
    def forward(ctx, group, X):
        ctx.group = group
        ctx.save_for_backward(X.detach())
        group.x.copy_(X.detach().reshape(group.T, group.d))
        group._launch(_lib.STEP_FORWARD)
        return group.moments.clone()

    @staticmethod
    def backward(ctx, g):
        group = ctx.group
        (X,) = ctx.saved_tensors
        group.x.copy_(X.reshape(group.T, group.d))      # (another evaluation may have used the group since the forward)
        group.seeds.copy_(g)
        group._launch(_lib.STEP_INPUT_GRADIENTS)
        return None, group.gx.sum(0).reshape(X.shape)


class PredictGroup:
    _noise = None

    @classmethod
    def why_not(cls, model, fidelity, T, d, on_gpu=True):
        """None when ``model``'s predictive moments at T test points up to layer ``fidelity`` fit this class's kernel, else
        the reason as a sentence (``on_gpu=False``: the parameters may be on the host).  The constructor's own gate."""
        raise NotImplementedError

    def freeze(self):
        """The parameters are constants until ``thaw()`` (an acquisition search): a group that keeps chains forms them once."""

    def thaw(self):
        """Ends ``freeze()``; harmless without one.  May synchronise and report what the launches since left behind."""

    @contextlib.contextmanager
    def frozen(self):
        self.freeze()
        try:
            yield self
        finally:
            self.thaw()

    def moments_at(self, X):
        """(n_models, 2, T S) (T for fidelity 0): mean and variance of the top layer's columns, WITHOUT the likelihood noise;
        differentiable w.r.t. X."""
        X = X.reshape(self.T, self.d)
        if X.requires_grad and torch.is_grad_enabled():
            return _MomentsFn.apply(self, X)
        self.x.copy_(X.detach())
        self._launch(_lib.STEP_FORWARD)
        return self.moments.clone()

    def noise(self, refresh=False):
        """(n_models,) likelihood noise of the top layer (constrained values).  The parameters are constants while a group is
        in use (an acquisition search against fitted models), so the values are formed once; ``refresh=True`` re-reads them."""
        if refresh or self._noise is None:
            with torch.no_grad():
                self._noise = torch.stack([getattr(m, m.name_hidden_layer_likelihood + str(self.fidelity)).noise.reshape(())
                                           for m in self.models])
        return self._noise

    def acquisition_moments(self, X):
        """(mus, vars), each (n_models, T): MFDGP.predict_for_acquisition of every model (noise added, moments over the S
        fixed samples, mfdgp.py:237-262)."""
        mom = self.moments_at(X)
        mean, var = mom[:, 0], mom[:, 1] + self.noise()[:, None]
        if self.fidelity == 0:
            return mean, var
        n = mean.shape[0]
        mu = mean.reshape(n, self.T, self.S)
        mus = mu.mean(2)
        second = (var.reshape(n, self.T, self.S) + mu * mu).mean(2)
        return mus, second - mus * mus
