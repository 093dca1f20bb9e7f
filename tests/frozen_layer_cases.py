"""The calls pinned bitwise by tests/golden/frozen_layer_bits.npz (tools/record_frozen_layer_golden.py writes it,
tests/test_hip_layer.py and tests/test_hip_overlap.py compare against it): a layer's frozen CHAIN state and the PANEL calls
against it, through functional.freeze_chain / layer_panel_frozen / predictive_covariance, and a three-layer model's
predict_for_acquisition inside MFDGP.frozen_chains().  Every input comes from synthetic.make_problem or a seeded generator.

Keys of ``layer_arrays()`` -- kind k in (0, 1), M in (20, 150), branch b in (0, 1), nbase n in (7, 200) with xdiv = 5:
  "M<M>/k<k>/b<b>/state"         fc.state (M = 20), or its SHA-256 as four words (M = 150: six 160 x 160 matrices per chain
                                 would not fit a committed fixture)
  "M<M>/k<k>/b<b>/kl", ".../info"
  "M<M>/k<k>/b<b>/n<n>/mean", ".../var", ".../g_x", ".../g_f" (kind 1)   layer_panel_frozen and its backward with want_dx
  "M<M>/k<k>/cov"                predictive_covariance at N' = 35 against the eval-branch chain
Keys of ``model_arrays()``: "model/f<1|2>/mus", ".../vs", ".../dX" (dX of mus.sum() + 3 vs.sum()) at T = 7, M = 33.
"""
import hashlib

import numpy as np
import torch

from mobocmf_amd import functional as F
from mobocmf_amd import gp
from mobocmf_amd.util import synthetic

D, XDIV = 3, 5
MS, NBASES = (20, 150), (7, 200)
DEV = "cuda"


def bits(t):
    """int64 bit pattern (CPU) of a float64 / uint8 tensor; an int32 scalar is widened."""
    t = t.detach().cpu().contiguous()
    return t.to(torch.int64).reshape(1) if t.dtype == torch.int32 else t.view(torch.int64)


def _digest(state):
    return torch.from_numpy(np.frombuffer(hashlib.sha256(state.cpu().numpy().tobytes()).digest(), dtype=np.int64).copy())


def layer_arrays():
    """(pinned, state_after): name -> int64 tensor; ``state_after[name]`` is "<...>/state" read again after every PANEL
    forward and backward against that chain (a frozen state is read-only)."""
    out, after = {}, {}
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64, device=DEV)
    for M in MS:
        model = synthetic.model_from_problem(synthetic.make_problem(d=D, L=2, M=M, N=M + 10, S=1, seed=M), device=DEV)
        for kind, layer in enumerate(model._layers()):
            vs = layer.variational_strategy
            vd = vs._variational_distribution
            hyp = gp.pack_hypers(layer.covar_module, layer.kind)
            assert layer.kind == kind
            for branch in (0, 1):
                key = "M%d/k%d/b%d" % (M, kind, branch)
                fc = F.freeze_chain(vs.Zx, vs.zf if kind == 1 else None, hyp, vd.variational_mean, vd.chol_variational_covar,
                                    kind, branch=branch)
                state = fc.state.clone()
                out[key + "/state"] = bits(state) if M == 20 else _digest(state)
                out[key + "/kl"], out[key + "/info"] = bits(fc.kl), bits(fc.info)
                for nbase in NBASES:
                    prob = synthetic.make_problem(d=D, L=2, M=4, N=nbase, S=XDIV, seed=300 + nbase)
                    x = t(prob["x"]).requires_grad_(True)
                    f = t(prob["eps"][1]).requires_grad_(True) if kind == 1 else None
                    g = torch.Generator().manual_seed(1000 * M + 10 * nbase + 2 * kind + branch)
                    gm, gv = (torch.randn(nbase * XDIV, dtype=torch.float64, generator=g).to(DEV) for _ in range(2))
                    mean, var = F.layer_panel_frozen(fc, x, f, xdiv=XDIV, want_dx=True)
                    torch.autograd.backward([mean, var], [gm, gv])
                    sub = "%s/n%d" % (key, nbase)
                    out[sub + "/mean"], out[sub + "/var"], out[sub + "/g_x"] = bits(mean), bits(var), bits(x.grad)
                    if kind == 1:
                        out[sub + "/g_f"] = bits(f.grad)
                    if branch == 1 and nbase == NBASES[0]:
                        _, cov = F.predictive_covariance(x.detach(), None if f is None else f.detach(), vs.Zx,
                                                         vs.zf if kind == 1 else None, hyp, None, None, kind, xdiv=XDIV,
                                                         chain=fc)
                        out["M%d/k%d/cov" % (M, kind)] = bits(cov)
                torch.cuda.synchronize()
                after[key + "/state"] = bits(fc.state) if M == 20 else _digest(fc.state)
    return out, after


def model_arrays():
    prob = synthetic.make_problem(d=D, L=3, M=33, N=50, S=5, seed=8)
    model = synthetic.model_from_problem(prob, num_samples_for_training=1, num_samples_for_acquisition=5, device=DEV)
    X = torch.as_tensor(synthetic.make_problem(d=D, L=2, M=4, N=7, S=1, seed=77)["x"], dtype=torch.float64, device=DEV)
    out = {}
    with model.frozen_chains():
        for fidelity in (1, 2):
            Xr = X.clone().requires_grad_(True)
            mus, vs = model.predict_for_acquisition(Xr, fidelity)
            (mus.sum() + 3.0 * vs.sum()).backward()
            for name, v in (("mus", mus), ("vs", vs), ("dX", Xr.grad)):
                out["model/f%d/%s" % (fidelity, name)] = bits(v)
    return out
