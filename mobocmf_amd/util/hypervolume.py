"""``HV(ref_point=...)``: the call form of ``pymoo.indicators.hv.HV`` that the reference's BO driver scores its recommendation
with (examples/toy_synthetic_2D_JESMOCMF: ``HV(ref_point=np.array([1000.0, 1000.0]))(F)``), on this build's kernels.

Like pymoo (``nds=True``) only the non-dominated points count: the points that weakly dominate the reference point are
reduced to their front on the device (``functional.pareto_mask``), whose exact hypervolume is then computed there
(``functional.hypervolume``).  Dominated points add no volume, so this changes the work, not the value.  There is no CPU
fallback: without a gfx950 device every call raises ``MobocmfError``.
"""
import numpy as np
import torch

from .. import _lib


class HV:

    def __init__(self, ref_point):
        self.ref_point = np.asarray(ref_point, dtype=np.float64).reshape(-1)
        if self.ref_point.size < 1 or self.ref_point.size > _lib.HV_MAX_K:
            raise _lib.MobocmfError("HV: the reference point has 1..%d objectives" % _lib.HV_MAX_K)

    def __call__(self, F):
        return self.do(F)

    def do(self, F):
        """Hypervolume of the rows of ``F`` ((n, k) numpy array or torch tensor; one point may be given as (k,))."""
        from .. import functional
        _lib.require_device()
        dev = torch.device("cuda", torch.cuda.current_device())
        F = torch.as_tensor(F).detach().to(device=dev, dtype=torch.float64)
        if F.dim() == 1:
            F = F[None, :]
        k = self.ref_point.size
        if F.dim() != 2 or F.shape[1] != k:
            raise _lib.MobocmfError("HV: expected (n, %d) objective values, got %s" % (k, tuple(F.shape)))
        if F.shape[0] == 0:
            return functional.hypervolume(F, self.ref_point)
        if bool(torch.isnan(F).any()):
            raise _lib.MobocmfError("HV: NaN objective values")
        ref = torch.from_numpy(self.ref_point).to(dev)
        F = F[(F <= ref).all(1)]
        mask, _ = functional.pareto_mask(F.T)
        return functional.hypervolume(F[mask], self.ref_point)
