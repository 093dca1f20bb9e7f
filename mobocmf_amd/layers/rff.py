"""Random-Fourier-feature function samples from the prior / the variational posterior of an MFDGP layer
(reference: mobocmf/layers/mfdgp_hidden_layer.py:288-514, numpy host code there as well).

Weight-space view: f(x) = theta^T phi(x), phi(x) = sqrt(2 a / F) cos(W x + b) with W ~ N(0, 1) / lengthscale,
b ~ U(0, 2 pi).  Layer >= 1 kernel a1 E1(x) (nu f f' + af Ef(f)) + a2 E2(x) has the feature map
[ sqrt(nu) f phi_x1(x) ; phi_{x1 f}([x, f]) ; phi_x2(x) ]  (3F features; the middle block is the RBF on [x, f] with
outputscale a1*af, sharing W_x1 and b_x1 with the first block, as the reference does).
Posterior weights given q(u) = N(m, S) at the inducing inputs:  A = Phi Phi^T + s2 I,
theta ~ N( A^-1 Phi m ,  s2 A^-1 + A^-1 Phi S Phi^T A^-1 ), drawn by Matheron's rule with M x M algebra.

The weights are drawn on the host in float64 (M x M algebra, not part of the ELBO hot path).  The returned callables take a
numpy array (n, d) or (d,), like the reference's, and recurse through the previous layer's sample; large batches (the
Pareto grid of MOOP, 1000 d^2 rows) are evaluated on the model's GPU by the HIP kernel ``mobocmf_rff_eval`` (one launch per
layer, the F x n feature matrix never materialised), single points and gradients on the host.
"""
import math

import numpy as np
import torch


def _phi(x, W, b, alpha):
    """(F, n) feature matrix."""
    F = W.shape[0]
    return math.sqrt(2.0 * alpha / F) * torch.cos(W @ x.T + b)


def _posterior_weights(Phi, m, Ls, sigma2, gen):
    """One draw of theta ~ N(A^-1 Phi m, s2 A^-1 + A^-1 Phi S Phi^T A^-1), A = Phi Phi^T + s2 I, S = Ls Ls^T -- the
    distribution the reference samples with F x F factorisations (mfdgp_hidden_layer.py:296-307) -- by Matheron's
    rule in the M-dimensional function space (M inducing points << F features):

        theta = theta0 + Phi (Phi^T Phi + s2 I)^-1 (u - Phi^T theta0 - e),   theta0 ~ N(0, I_F), u ~ N(m, S), e ~ N(0, s2 I_M)

    Same mean (push-through identity) and covariance (s2 A^-1 from the prior draw, A^-1 Phi S Phi^T A^-1 from u);
    O(F M^2) instead of O(F^3)."""
    nF, M = Phi.shape
    rn = lambda n: torch.randn(n, dtype=Phi.dtype, generator=gen)
    theta0, z, e = rn(nF), rn(M), rn(M) * math.sqrt(sigma2)
    u = m + Ls @ z
    G = Phi.T @ Phi
    eye = torch.eye(M, dtype=Phi.dtype)
    jit = sigma2
    for i in range(6):
        Lg, info = torch.linalg.cholesky_ex(G + jit * eye)
        if int(info) == 0:
            break
        jit = sigma2 + 1e-10 * 10 ** i
    rhs = u - Phi.T @ theta0 - e
    return theta0 + Phi @ torch.cholesky_solve(rhs[:, None], Lg)[:, 0]


GRID_ROWS_ON_DEVICE = 4096      # batches at least this large are evaluated on the sample's device (the Pareto grid)


class _OnDevice:
    """Tensors of a sample, mirrored lazily on the devices they are evaluated on."""

    def __init__(self, **tensors):
        self._t = {torch.device("cpu"): tensors}

    def on(self, dev):
        dev = torch.device(dev)
        if dev not in self._t:
            self._t[dev] = {k: v.to(dev) for k, v in self._t[torch.device("cpu")].items()}
        return self._t[dev]


def _as_callable(feature_fn, theta, prev, device=None, kernel_args=None):
    """f(x, gradient=False): numpy in, numpy out -- (n,) values, or the (d,) gradient for a single point.
    Single points (the SLSQP refinements) stay on the host; grids of >= GRID_ROWS_ON_DEVICE rows run on ``device`` through
    the HIP kernel (``kernel_args``: kind, the feature tensors and the three scale factors)."""
    th = _OnDevice(theta=theta)

    def evaluate(xt):
        f_prev = prev._torch(xt) if prev is not None else None
        return th.on(xt.device)["theta"] @ feature_fn(xt, f_prev)

    def evaluate_device(xd):
        """xd (n, d) on the GPU -> the sample's values there (layer recursion: the previous sample first)."""
        from .. import functional as F
        kind, P, scales = kernel_args
        p = P.on(xd.device)
        f_prev = prev._device(xd) if prev is not None else None
        return F.rff_eval(kind, xd, f_prev, p["W1"], p["b1"].reshape(-1), p.get("Wf"), p.get("W2"),
                          None if "b2" not in p else p["b2"].reshape(-1), th.on(xd.device)["theta"], *scales)

    def wrapper(x, gradient=False):
        xt = torch.as_tensor(np.asarray(x), dtype=torch.float64)
        if xt.dim() == 1:
            xt = xt[None, :]
        if gradient:
            assert xt.shape[0] == 1, "the gradient is defined for a single point (as in the reference)"
            xt = xt.clone().requires_grad_(True)
            (g,) = torch.autograd.grad(evaluate(xt).sum(), xt)
            return g[0].numpy()
        with torch.no_grad():
            if device is not None and kernel_args is not None and xt.shape[0] >= GRID_ROWS_ON_DEVICE:
                return evaluate_device(xt.to(device).contiguous()).cpu().numpy()
            return evaluate(xt).numpy()

    wrapper._torch = evaluate
    wrapper._device = evaluate_device
    return wrapper


def _hypers(layer):
    cm = layer.covar_module
    g = lambda t: t.detach().cpu().double()
    if layer.num_layer == 0:
        return {"ls": g(cm.base_kernel.lengthscale).reshape(-1), "alpha": float(g(cm.outputscale))}
    k1, kf = cm.kernels[0].kernels[0], cm.kernels[0].kernels[1].kernels[1]
    kl, k2 = cm.kernels[0].kernels[1].kernels[0], cm.kernels[1]
    return {"ls1": g(k1.base_kernel.lengthscale).reshape(-1), "a1": float(g(k1.outputscale)),
            "lsf": g(kf.base_kernel.lengthscale).reshape(-1), "af": float(g(kf.outputscale)),
            "ls2": g(k2.base_kernel.lengthscale).reshape(-1), "a2": float(g(k2.outputscale)),
            "nu": float(g(kl.variance))}


def _draw_features(h, d, F, gen, layer0):
    """Returns (feature function for host torch, kernel_args = (kind, tensors, (s0, s1, s2)) for mobocmf_rff_eval)."""
    rn = lambda *s: torch.randn(*s, dtype=torch.float64, generator=gen)
    ru = lambda *s: 2.0 * math.pi * torch.rand(*s, dtype=torch.float64, generator=gen)
    if layer0:
        P = _OnDevice(W1=rn(F, d) / h["ls"], b1=ru(F, 1))

        def feats0(x, f):
            p = P.on(x.device)
            return _phi(x, p["W1"], p["b1"], h["alpha"])

        return feats0, (0, P, (math.sqrt(2.0 * h["alpha"] / F), 0.0, 0.0))
    W1, Wf, W2 = rn(F, d) / h["ls1"], rn(F) / h["lsf"], rn(F, d) / h["ls2"]
    b1, b2 = ru(F, 1), ru(F, 1)
    P = _OnDevice(W1=W1, W2=W2, b1=b1, b2=b2, Wf=Wf, W1f=torch.cat([W1, Wf[:, None]], 1))

    def feats(x, f):
        p = P.on(x.device)
        xf = torch.cat([x, f[:, None]], 1)
        return torch.cat([_phi(x, p["W1"], p["b1"], h["a1"]) * f * math.sqrt(h["nu"]),
                          _phi(xf, p["W1f"], p["b1"], h["a1"] * h["af"]), _phi(x, p["W2"], p["b2"], h["a2"])], 0)

    scales = (math.sqrt(2.0 * h["a1"] * h["nu"] / F), math.sqrt(2.0 * h["a1"] * h["af"] / F), math.sqrt(2.0 * h["a2"] / F))
    return feats, (1, P, scales)


def _posterior_layer(layer, input_dim, nFeatures, sigma2, generator):
    """The draws of one layer's posterior sample, in the generator order both samplers below share: the features, then
    Matheron's rule.  Returns (hyper-parameters, feature function, kernel_args, theta)."""
    h = _hypers(layer)
    vs = layer.variational_strategy
    Z = vs.inducing_points.detach().cpu().double()
    vd = vs._variational_distribution
    m = vd.variational_mean.detach().cpu().double()
    Ls = torch.tril(vd.chol_variational_covar.detach().cpu().double())
    feats, kargs = _draw_features(h, input_dim, nFeatures, generator, layer.num_layer == 0)
    if layer.num_layer == 0:
        Phi = feats(Z, None)
    else:
        Phi = feats(Z[:, :-1], Z[:, -1])          # the f column of Z~ is the previous layer's variational mean
    theta = _posterior_weights(Phi, m, Ls, sigma2, generator)
    return h, feats, kargs, theta


def sample_from_posterior(layer, input_dim, prev_sample=None, nFeatures=500, sigma2=1e-6, generator=None, device=None):
    """One function sample from the layer's variational posterior (reference :309-337 layer 0, :364-444 layer >= 1)."""
    assert (prev_sample is None) == (layer.num_layer == 0)
    _, feats, kargs, theta = _posterior_layer(layer, input_dim, nFeatures, sigma2, generator)
    return _as_callable(feats, theta, prev_sample, device, kargs)


def sample_from_prior(layer, input_dim, prev_sample=None, nFeatures=500, generator=None, device=None):
    """One function sample from the synthetic-problem prior (reference :339-362, :446-514: fixed test hyper-parameters
    lengthscale 0.25 d (x10 for x1), outputscales 1 / 1 / 0.01, nu 1)."""
    d = input_dim
    if layer.num_layer == 0:
        h = {"ls": torch.full((d,), 0.25 * d, dtype=torch.float64), "alpha": 1.0}
    else:
        h = {"ls1": torch.full((d,), 2.5 * d, dtype=torch.float64), "a1": 1.0, "lsf": torch.ones(1, dtype=torch.float64),
             "af": 1.0, "ls2": torch.full((d,), 0.25 * d, dtype=torch.float64), "a2": 0.01, "nu": 1.0}
    feats, kargs = _draw_features(h, d, nFeatures, generator, layer.num_layer == 0)
    nF = nFeatures if layer.num_layer == 0 else 3 * nFeatures
    theta = torch.randn(nF, dtype=torch.float64, generator=generator)
    return _as_callable(feats, theta, prev_sample, device, kargs)


# ---------------------------------------------------------------------------------------------------------------
# Portable chain samples: the whole function sample of one black-box (layer 0 and the layers >= 1 recursing on it) as
# plain tensors, so that it can be packed into one float64 buffer, exchanged between ranks, and evaluated for several
# black-boxes at once on a grid (mobocmf_rff_eval_chains).
# ---------------------------------------------------------------------------------------------------------------
PACK_VERSION = 1
_HEAD = 5          # version, L, d, F, length; then the L layer kinds
_LAYER_HEAD = 7    # alpha (kind 0) or a1, af, a2, nu (kind 1, zero padded to 4), then s0, s1, s2


def packed_length(L, d, F):
    """Doubles of a packed chain sample of L layers: 5 + L + 7 L + F (d + 2) for layer 0 + F (2 d + 6) per layer above it
    (128 KB for L = 2, d = 8, F = 500)."""
    return _HEAD + L + _LAYER_HEAD * L + F * (d + 2) + (L - 1) * F * (2 * d + 6)


def _layer_operands(kind, d, F):
    """(name, numel) of a layer's operands in packed order."""
    ops = [("W1", F * d), ("b1", F), ("theta", F if kind == 0 else 3 * F)]
    return ops + ([("Wf", F), ("W2", F * d), ("b2", F)] if kind == 1 else [])


class RFFChainSample:
    """One black-box's posterior function sample with every layer held as tensors: per layer ``kind`` (0: layer 0, 1: the
    layers above it), the host feature maps' hyper-parameters (``alpha``, or ``a1, af, a2, nu``), the three kernel scales of
    ``mobocmf_rff_eval`` and the draws ``W1, b1, theta`` (+ ``Wf, W2, b2`` for kind 1); the lengthscales are folded into the W.

    The callable interface of ``sample_function_from_each_layer``'s top layer: ``f(x)`` -> (n,) values, ``f(x, gradient=True)``
    -> the (d,) gradient at one point, ``f._torch`` (host torch, autograd) and ``f._device`` (GPU tensor in and out); grids of
    >= GRID_ROWS_ON_DEVICE rows run on ``device`` (the chained kernel, all layers in one launch).  Survives deepcopy and dill;
    ``pack()`` / ``unpack()`` round-trip bitwise."""

    def __init__(self, layers, d, device=None):
        self.layers = layers
        self.d = int(d)
        self.F = int(layers[0]["F"])
        self.device = None if device is None else torch.device(device)
        self._dev = {}

    def __getstate__(self):
        st = self.__dict__.copy()
        st["_dev"] = {}              # device mirrors are rebuilt on first use
        return st

    # ------------------------------------------------------------------ host evaluation (the per-layer callables' maths)
    def _on(self, dev):
        dev = torch.device(dev)
        if dev.type == "cpu":
            return self.layers
        if dev not in self._dev:
            self._dev[dev] = [{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in L.items()} for L in self.layers]
        return self._dev[dev]

    def _torch(self, x):
        f = None
        for L in self._on(x.device):
            F = L["F"]
            if L["kind"] == 0:
                phi = _phi(x, L["W1"], L["b1"][:, None], L["alpha"])
            else:
                W1f = torch.cat([L["W1"], L["Wf"][:, None]], 1)
                xf = torch.cat([x, f[:, None]], 1)
                phi = torch.cat([_phi(x, L["W1"], L["b1"][:, None], L["a1"]) * f * math.sqrt(L["nu"]),
                                 _phi(xf, W1f, L["b1"][:, None], L["a1"] * L["af"]),
                                 _phi(x, L["W2"], L["b2"][:, None], L["a2"])], 0)
            assert phi.shape[0] == (F if L["kind"] == 0 else 3 * F)
            f = L["theta"] @ phi
        return f

    # ------------------------------------------------------------------ device evaluation
    def device_operands(self, device):
        """(params, layers) of this sample for ``functional.rff_eval_chains``: the packed buffer on ``device`` and the
        per-layer offsets into it (cached)."""
        dev = torch.device(device)
        key = ("packed", dev)
        if key not in self._dev:
            buf = self.pack()
            self._dev[key] = (buf.to(dev), self.layer_offsets(0))
        return self._dev[key]

    def layer_offsets(self, base):
        """Per layer: kind, F, scales and the operand offsets (into a buffer holding this packed sample at ``base``)."""
        out, off = [], base + _HEAD + len(self.layers)
        for L in self.layers:
            e = {"kind": L["kind"], "F": L["F"], "s0": L["scales"][0], "s1": L["scales"][1], "s2": L["scales"][2]}
            off += _LAYER_HEAD
            for name, cnt in _layer_operands(L["kind"], self.d, L["F"]):
                e[name] = off
                off += cnt
            out.append(e)
        return out

    def _device(self, xd):
        from .. import functional as Fn
        params, layers = self.device_operands(xd.device)
        return Fn.rff_eval_chains(xd, params, [layers])[0]

    def value_and_grad(self, xd):
        """xd (n, d) on the GPU -> (values (n,), input gradients (n, d)) there, every row in one launch
        (mobocmf_rff_chains_value_grad)."""
        from .. import functional as Fn
        params, layers = self.device_operands(xd.device)
        vals, grads = Fn.rff_chains_value_grad(xd, params, [layers])
        return vals[0], grads[0]

    def __call__(self, x, gradient=False):
        xt = torch.as_tensor(np.asarray(x), dtype=torch.float64)
        if xt.dim() == 1:
            xt = xt[None, :]
        if gradient:
            assert xt.shape[0] == 1, "the gradient is defined for a single point (as in the reference)"
            xt = xt.clone().requires_grad_(True)
            (g,) = torch.autograd.grad(self._torch(xt).sum(), xt)
            return g[0].numpy()
        with torch.no_grad():
            if self.device is not None and self.device.type == "cuda" and xt.shape[0] >= GRID_ROWS_ON_DEVICE:
                return self._device(xt.to(self.device).contiguous()).cpu().numpy()
            return self._torch(xt).numpy()

    def negated(self):
        """The sample -f: the same layers with the top layer's ``theta`` negated (a maximised objective handed to a MOOP,
        which minimises)."""
        layers = [dict(L) for L in self.layers]
        layers[-1]["theta"] = -layers[-1]["theta"]
        return RFFChainSample(layers, self.d, self.device)

    # ------------------------------------------------------------------ packing
    def pack(self):
        """1-D float64 CPU tensor: header (version, L, d, F, length, the L kinds), then per layer its 7 scalars and the
        operands in the order W1, b1, theta[, Wf, W2, b2].  Length: ``packed_length``."""
        L, d, F = len(self.layers), self.d, self.F
        n = packed_length(L, d, F)
        parts = [torch.tensor([PACK_VERSION, L, d, F, n] + [Lr["kind"] for Lr in self.layers], dtype=torch.float64)]
        for Lr in self.layers:
            hyp = [Lr["alpha"], 0.0, 0.0, 0.0] if Lr["kind"] == 0 else [Lr["a1"], Lr["af"], Lr["a2"], Lr["nu"]]
            parts.append(torch.tensor(hyp + list(Lr["scales"]), dtype=torch.float64))
            parts += [Lr[name].reshape(-1).to(torch.float64) for name, _ in _layer_operands(Lr["kind"], d, F)]
        buf = torch.cat(parts)
        assert buf.numel() == n
        return buf

    @staticmethod
    def header(buf):
        """(version, L, d, F, length) of a packed buffer (padding after ``length`` is ignored)."""
        h = buf[:_HEAD].tolist()
        return tuple(int(v) for v in h)

    @classmethod
    def unpack(cls, buf, device=None):
        buf = torch.as_tensor(buf).detach().to("cpu", torch.float64).reshape(-1)
        ver, L, d, F, n = cls.header(buf)
        if ver != PACK_VERSION or L < 1 or d < 1 or F < 1 or n != packed_length(L, d, F) or buf.numel() < n:
            raise ValueError("RFFChainSample.unpack: not a packed chain sample (header %s)" % ((ver, L, d, F, n),))
        kinds = [int(v) for v in buf[_HEAD:_HEAD + L].tolist()]
        off, layers = _HEAD + L, []
        for kind in kinds:
            sc = buf[off:off + _LAYER_HEAD].tolist()
            off += _LAYER_HEAD
            Lr = {"kind": kind, "F": F, "scales": tuple(sc[4:7])}
            if kind == 0:
                Lr["alpha"] = sc[0]
            else:
                Lr["a1"], Lr["af"], Lr["a2"], Lr["nu"] = sc[:4]
            for name, cnt in _layer_operands(kind, d, F):
                t = buf[off:off + cnt].clone()
                Lr[name] = t.reshape(F, d) if name in ("W1", "W2") else t
                off += cnt
            layers.append(Lr)
        return cls(layers, d, device)


def sample_chain_from_posterior(model, nFeatures=500, sigma2=1e-6, generator=None, device=None):
    """The top-layer sample of ``model.sample_function_from_each_layer`` as an ``RFFChainSample``: the same maths and the
    same generator calls in the same order, so one generator state gives the same function either way.  ``device``:
    default the model's GPU (None on the CPU)."""
    layers = []
    for layer in model._layers():
        h, _, (kind, P, scales), theta = _posterior_layer(layer, model.input_dims, nFeatures, sigma2, generator)
        p = P.on("cpu")
        Lr = {"kind": kind, "F": nFeatures, "scales": tuple(float(s) for s in scales), "theta": theta,
              "W1": p["W1"], "b1": p["b1"].reshape(-1)}
        if kind == 0:
            Lr["alpha"] = float(h["alpha"])
        else:
            Lr.update(a1=float(h["a1"]), af=float(h["af"]), a2=float(h["a2"]), nu=float(h["nu"]), Wf=p["Wf"],
                      W2=p["W2"], b2=p["b2"].reshape(-1))
        layers.append(Lr)
    return RFFChainSample(layers, model.input_dims, model._sample_device() if device is None else device)
