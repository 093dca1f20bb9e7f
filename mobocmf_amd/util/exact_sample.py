"""Posterior function samples of the exact-GP baselines (models/mfgp.py: ``MFGP``, ``MFGP_lin``) as ``RFFChainSample``s: the
stage of a max-value entropy search iteration between the fit and the acquisition search (csrc/exact_sample.hip,
include/mobocmf_hip.h: mobocmf_exact_sample_*).

Both kernels are  k([x, t], [x', t']) = s(t) s(t') k_sig(x, x') + ntab[min(t, t')] k_noi(x, x')  with a non-decreasing ntab,
ntab[m] = sum_{l <= m} delta_l.  With F random features per ARD-RBF kernel, C = cos(W x + b) (F x n) and c = sqrt(2 a / F), the
weight-space feature map has (1 + n_levels) F rows: block 0 is s(l_i) c_sig C_sig[:, i], block 1 + l is sqrt(delta_l) c_noi
C_noi[:, i] on the rows with l_i >= l.  Matheron's rule in the n-dimensional function space (layers/rff.py: _posterior_weights),

    G = Phi^T Phi + noise I,   r = y - Phi^T theta0 - e,   w = G^-1 r,   theta = theta0 + Phi w,

and the function at output level f is ONE random-feature layer of 2F features,

    g_f(x) = s(f) c_sig theta_sig . cos(W_sig x + b_sig) + c_noi (sum_{l <= f} sqrt(delta_l) theta_noi,l) . cos(W_noi x + b_noi):

a kind-0 layer with W1 = [W_sig; W_noi], the scales folded into theta, s0 = 1 and alpha = s0^2 F' / 2 = F, which the host
evaluation (``RFFChainSample._torch``) and the kernels evaluate as the same function.

The draws, in this order, on the generator's device (``generator=None``: the model's device, its default generator):

    W_sig = randn(F, d) / ls_sig,  b_sig = 2 pi rand(F),  W_noi = randn(F, d) / ls_noi,  b_noi = 2 pi rand(F),
    theta0 = randn((1 + n_levels) F),  e = sqrt(noise) randn(n)

``engine="device"``: G and r of ALL models in one launch, mobocmf_exact_gp_factor per model, w / theta / the packed samples in
one more call, and ONE device-to-host copy (the packed samples with the factorisations' info words).  ``engine="host"``: the
same algebra in float64 torch on the CPU from the same draws.
"""
import ctypes
import math

import torch

from .. import _lib
from ..layers.rff import RFFChainSample, packed_length

MAX_N, MAX_PROBLEMS = _lib.EXACT_SAMPLE_MAX_N, _lib.EXACT_SAMPLE_MAX_PROBLEMS


def why_not(model, on_gpu=True):
    """None when ``model`` fits the device draw, else the reason as a sentence: the limits of ``ExactGPPredictGroup.why_not``."""
    from .exact_predict import why_not as predict_why_not
    d = getattr(model, "input_dim", 0)
    return predict_why_not(model, 0, 1, d, on_gpu=on_gpu)


def level_tables(model):
    """(sig, ntab, sqd) of ``model``'s kernel on its device, n_levels each: the signal factor s(level), the noise factor of a
    min-level and sqrt(delta_l), delta_0 = ntab[0], delta_l = ntab[l] - ntab[l - 1].  No host read."""
    cm, d, nl = model.covar_module, model.input_dim, model.num_fidelities
    dev = model.x_train.device
    with torch.no_grad():
        rows = torch.zeros(nl, d + 1, dtype=torch.float64, device=dev)
        rows[:, d] = torch.arange(nl, dtype=torch.float64, device=dev)
        _, sig = cm.hip_factors(rows)
        sig = torch.ones(nl, dtype=torch.float64, device=dev) if sig is None else sig.to(torch.float64).contiguous()
        ntab = cm.hip_noise_table(nl, dev).to(torch.float64).contiguous()
        delta = ntab - torch.cat([ntab.new_zeros(1), ntab[:-1]])
        sqd = delta.clamp_min(0.0).sqrt().contiguous()
    return sig, ntab, sqd


def model_operands(model):
    """What the draw reads of a fitted model, on its device: x (n x d), lev (n, int32), y (n), sig, ntab, sqd (n_levels),
    scal = [a_sig, a_noi, noise], ls_sig, ls_noi (d)."""
    cm, d = model.covar_module, model.input_dim
    with torch.no_grad():
        sig, ntab, sqd = level_tables(model)
        ks, kn = cm.cov_funct_signal, cm.cov_funct_noise
        return dict(x=model.x_train[:, :d].contiguous(), lev=cm.hip_factors(model.x_train)[0].contiguous(),
                    y=model.y_train.reshape(-1).contiguous(), sig=sig, ntab=ntab, sqd=sqd,
                    scal=torch.stack([ks.outputscale.reshape(()), kn.outputscale.reshape(()),
                                      model.likelihood.noise.reshape(())]).detach().to(torch.float64).contiguous(),
                    ls_sig=ks.base_kernel.lengthscale.detach().reshape(-1).to(torch.float64),
                    ls_noi=kn.base_kernel.lengthscale.detach().reshape(-1).to(torch.float64))


def draw_operands(model, nFeatures, generator=None, ops=None):
    """The random operands of one draw in the module's documented order, on the model's device:
    dict(W_sig, b_sig, W_noi, b_noi, theta0, e)."""
    ops = model_operands(model) if ops is None else ops
    dev = ops["x"].device
    gdev = dev if generator is None else generator.device
    F, d, nl, n = int(nFeatures), ops["x"].shape[1], ops["sig"].numel(), ops["x"].shape[0]
    rn = lambda *s: torch.randn(*s, dtype=torch.float64, device=gdev, generator=generator).to(dev)
    ru = lambda *s: torch.rand(*s, dtype=torch.float64, device=gdev, generator=generator).to(dev)
    with torch.no_grad():
        W_sig, b_sig = rn(F, d) / ops["ls_sig"], 2.0 * math.pi * ru(F)
        W_noi, b_noi = rn(F, d) / ops["ls_noi"], 2.0 * math.pi * ru(F)
        theta0 = rn((1 + nl) * F)
        e = ops["scal"][2].sqrt() * rn(n)
    return dict(W_sig=W_sig.contiguous(), b_sig=b_sig, W_noi=W_noi.contiguous(), b_noi=b_noi, theta0=theta0, e=e.contiguous())


def fold(theta, level, sig, sqd, c_sig, c_noi, F):
    """theta' (2F) of output level ``level`` from theta ((1 + n_levels) F, block order)."""
    noi = sum(sqd[l] * theta[(1 + l) * F:(2 + l) * F] for l in range(level + 1))
    return torch.cat([sig[level] * c_sig * theta[:F], c_noi * noi])


def _chain_sample(W_sig, b_sig, W_noi, b_noi, theta_folded, device):
    F, d = W_sig.shape
    layer = {"kind": 0, "F": 2 * F, "scales": (1.0, 0.0, 0.0), "alpha": float(F), "W1": torch.cat([W_sig, W_noi], 0),
             "b1": torch.cat([b_sig, b_noi]), "theta": theta_folded}
    return RFFChainSample([layer], d, device)


class ChainDraw:
    """One model's draw: ``samples[level]`` the ``RFFChainSample``s, ``theta`` ((1 + n_levels) F, block order), ``w`` (n), the
    operands ``e`` (n) and ``noise``, ``engine`` and the factorisation's ``info`` (0).  With the device engine ``theta``,
    ``w``, ``e`` and ``noise`` are tensors on the GPU."""

    def __init__(self, samples, theta, w, e, noise, engine, info=0):
        self.samples, self.theta, self.w, self.e, self.noise, self.engine, self.info = samples, theta, w, e, noise, engine, info


def host_draw(ops, rnd, levels, device=None):
    """The host engine: Matheron's rule in float64 torch on the CPU from the operands ``ops`` (``model_operands``) and the draws
    ``rnd`` (``draw_operands``)."""
    from ..models.mfgp import gp_NotPSD
    c = lambda t: t.detach().to("cpu", torch.float64)
    x, lev, y = c(ops["x"]), ops["lev"].detach().cpu().long(), c(ops["y"])
    sig, sqd, scal = c(ops["sig"]), c(ops["sqd"]), c(ops["scal"])
    W_sig, b_sig, W_noi, b_noi = c(rnd["W_sig"]), c(rnd["b_sig"]), c(rnd["W_noi"]), c(rnd["b_noi"])
    theta0, e = c(rnd["theta0"]), c(rnd["e"])
    F, nl, n = W_sig.shape[0], sig.numel(), x.shape[0]
    if int(lev.min()) < 0 or int(lev.max()) >= nl:
        raise ValueError("a training row's fidelity level lies outside [0, %d)" % nl)
    c_sig, c_noi, noise = torch.sqrt(2.0 * scal[0] / F), torch.sqrt(2.0 * scal[1] / F), scal[2]
    C_sig, C_noi = torch.cos(W_sig @ x.T + b_sig[:, None]), torch.cos(W_noi @ x.T + b_noi[:, None])
    blocks = [sig[lev] * c_sig * C_sig] + [sqd[l] * c_noi * C_noi * (lev >= l).to(torch.float64) for l in range(nl)]
    Phi = torch.cat(blocks, 0)
    G = Phi.T @ Phi + noise * torch.eye(n, dtype=torch.float64)
    r = y - Phi.T @ theta0 - e
    Lg, info = torch.linalg.cholesky_ex(G)
    if int(info) != 0:
        raise gp_NotPSD("exact-GP function sample: Phi^T Phi + noise I is not positive definite (pivot %d)" % int(info))
    w = torch.cholesky_solve(r[:, None], Lg)[:, 0]
    theta = theta0 + Phi @ w
    samples = {int(f): _chain_sample(W_sig, b_sig, W_noi, b_noi, fold(theta, int(f), sig, sqd, c_sig, c_noi, F), device)
               for f in levels}
    return ChainDraw(samples, theta, w, e, float(noise), "host")


def _read_once(vals, words):
    from ..acquisition_functions.JESMOC_MFDGP import _read_once as read
    return read(vals, words)


class ExactSampleLaunch:
    """The device engine for SEVERAL (model, sample) problems: ``gram()`` (one launch: G and r of all problems),
    ``factorise()`` (mobocmf_exact_gp_factor per problem, r its right-hand side), ``weights()`` (w, theta and the packed
    samples) and ``read()``, the ONE device-to-host copy (the packed samples with the factorisations' info words), which
    returns the ``ChainDraw``s.  ``G(i)`` / ``r(i)`` / ``w(i)`` / ``theta(i)``: problem i's device tensors (npad x npad, n, n,
    (1 + n_levels) F).  ``ops_list`` / ``rnd_list``: per problem what ``model_operands`` / ``draw_operands`` return."""

    def __init__(self, ops_list, rnd_list, levels_list):
        lib = _lib.require_device()
        P = len(ops_list)
        if not 1 <= P <= MAX_PROBLEMS:
            raise _lib.MobocmfError("ExactSampleLaunch: 1 .. %d problems" % MAX_PROBLEMS)
        self.device = dev = ops_list[0]["x"].device
        self.host = host = (_lib.ExactSampleProblem * P)()
        self._words = words = torch.zeros(2, P, dtype=torch.int32, device=dev)      # the factorisations' info words | their copies
        mll = torch.zeros(P, dtype=torch.float64, device=dev)
        self._factor, self._outs = [], []
        sb, cb = ctypes.c_size_t(), ctypes.c_size_t()
        scratch_bytes = 0
        for i, (ops, rnd, levels) in enumerate(zip(ops_list, rnd_list, levels_list)):
            rec = host[i]
            n, d = ops["x"].shape
            nl, F = ops["sig"].numel(), rnd["W_sig"].shape[0]
            levels = [int(f) for f in levels]
            if len(levels) > _lib.EXACT_SAMPLE_MAX_LEVELS or any(not 0 <= f < nl for f in levels):
                raise ValueError("output levels %s of %d fidelity levels" % (levels, nl))
            if rnd["theta0"].numel() != (1 + nl) * F or rnd["e"].numel() != n or tuple(rnd["W_noi"].shape) != (F, d):
                raise ValueError("the draws do not have the model's shapes")
            npad, plen = (n + 127) // 128 * 128, packed_length(1, d, 2 * F)
            t = {k: v.to(dev).contiguous() for k, v in list(ops.items()) + list(rnd.items())}
            _lib.check(lib.mobocmf_exact_gp_workspace_bytes(n, 1, ctypes.byref(sb), ctypes.byref(cb)), "mobocmf_exact_gp_workspace_bytes")
            scratch_bytes = max(scratch_bytes, cb.value)
            z = lambda *s: torch.zeros(*s, dtype=torch.float64, device=dev)
            G, r, w, theta, chain = z(npad, npad), z(n), z(n), z((1 + nl) * F), z(max(len(levels), 1), plen)
            state = torch.zeros(sb.value, dtype=torch.uint8, device=dev)
            sv = state.view(torch.float64)
            rec.n, rec.d, rec.n_levels, rec.F, rec.n_out, rec.reserved = n, d, nl, F, len(levels), 0
            for o, f in enumerate(levels):
                rec.out_level[o] = f
            for name in ("x", "lev", "y", "sig", "ntab", "sqd", "scal", "W_sig", "b_sig", "W_noi", "b_noi", "theta0", "e"):
                setattr(rec, name, t[name].data_ptr())
            rec.G, rec.r, rec.w, rec.theta, rec.chain = G.data_ptr(), r.data_ptr(), w.data_ptr(), theta.data_ptr(), chain.data_ptr()
            rec.Linv, rec.a = sv[npad * npad:].data_ptr(), sv[2 * npad * npad:].data_ptr()      # (functional._exact_state_views)
            rec.info, rec.info_out = words[0, i:].data_ptr(), words[1, i:].data_ptr()
            self._factor.append((n, npad, G, r, state, sb.value, mll[i:], words[0, i:]))
            self._outs.append((levels, t, G, r, w, theta, chain, plen))
        self._scratch_bytes = scratch_bytes
        self._table = torch.zeros(ctypes.sizeof(host), dtype=torch.uint8, device=dev)
        self._table.copy_(torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8))

    def G(self, i):
        return self._outs[i][2]

    def r(self, i):
        return self._outs[i][3]

    def w(self, i):
        return self._outs[i][4]

    def theta(self, i):
        return self._outs[i][5]

    def gram(self):
        from .. import functional as Fn
        with torch.no_grad():
            Fn.exact_sample_gram(self.host, self._table)

    def factorise(self):
        from .. import functional as Fn
        lib = _lib.require_device()
        scratch = Fn.scratch_buffer(self._scratch_bytes, self.device)
        tune, stream = Fn.current_tuning(), Fn._stream()
        for n, npad, G, r, state, sbytes, m, info in self._factor:
            _lib.check(lib.mobocmf_exact_gp_factor(n, ctypes.c_void_p(G.data_ptr()), npad, ctypes.c_void_p(r.data_ptr()),
                                                   ctypes.c_void_p(m.data_ptr()), ctypes.c_void_p(info.data_ptr()),
                                                   ctypes.c_void_p(state.data_ptr()), sbytes, ctypes.c_void_p(scratch.data_ptr()),
                                                   scratch.numel(), ctypes.byref(tune), stream), "mobocmf_exact_gp_factor")

    def weights(self):
        from .. import functional as Fn
        with torch.no_grad():
            Fn.exact_sample_weights(self.host, self._table)

    def read(self):
        from .. import functional as Fn
        from ..models.mfgp import gp_NotPSD
        dev = self.device
        with torch.no_grad():
            flat, infos = _read_once(torch.cat([o[6].reshape(-1) for o in self._outs]), self._words[1])
        draws, off = [], 0
        for i, (levels, t, G, r, w, theta, chain, plen) in enumerate(self._outs):
            info = int(infos[i])
            Fn.raise_if_abandoned(info, "exact-GP function sample")
            if info != 0:
                raise gp_NotPSD("exact-GP function sample: Phi^T Phi + noise I is not positive definite (pivot %d)" % info)
            samples = {}
            for o, f in enumerate(levels):
                smp = RFFChainSample.unpack(flat[off + o * plen:off + (o + 1) * plen], dev)
                smp._dev[("packed", dev)] = (chain[o], smp.layer_offsets(0))      # (device_operands: no upload)
                samples[f] = smp
            off += chain.numel()
            draws.append(ChainDraw(samples, theta, w, t["e"], t["scal"][2], "device", info))
        return draws


def device_draw(ops_list, rnd_list, levels_list):
    """The device engine: one gram launch, one factorisation per problem, one weights call, one read.  Returns the
    ``ChainDraw``s."""
    launch = ExactSampleLaunch(ops_list, rnd_list, levels_list)
    launch.gram()
    launch.factorise()
    launch.weights()
    return launch.read()


class ChainDrawResult:
    """What ``draw_chain_samples`` returns: ``names`` (a dict's keys, a list's indices), ``engines[name]`` "host" or "device",
    ``draws[name]`` the ``ChainDraw`` and ``samples[name]`` the sample of the model's level (a dict level -> sample when
    several levels were asked for)."""

    def __init__(self, names):
        self.names, self.engines, self.draws, self.samples = list(names), {}, {}, {}


def draw_chain_samples(models, levels, nFeatures=500, generator=None, engine="device"):
    """One posterior function sample of each of SEVERAL exact GPs (a dict or a list, at most 64).  ``levels``: the output
    level(s) per model -- an int for all, or a dict / list with an int or a list of ints per model.  ``engine="device"``: the
    models ``why_not`` accepts together in the two launches of csrc/exact_sample.hip plus their factorisations, the others by
    the host engine one after the other (``result.engines[name]`` says which); ``"host"``: the host engine for all.  The models
    draw from ``generator`` in the order given."""
    if engine not in ("host", "device"):
        raise ValueError("draw_chain_samples: engine is \"host\" or \"device\" (got %r)" % (engine,))
    names = list(models.keys()) if isinstance(models, dict) else list(range(len(models)))
    mods = list(models.values()) if isinstance(models, dict) else list(models)
    if not 1 <= len(mods) <= MAX_PROBLEMS:
        raise _lib.MobocmfError("draw_chain_samples: 1 .. %d models" % MAX_PROBLEMS)
    per = lambda k, i: levels if isinstance(levels, int) else levels[k] if isinstance(levels, dict) else levels[i]
    lv = [per(k, i) for i, k in enumerate(names)]
    single = [isinstance(l, int) for l in lv]
    lv = [[l] if s else list(l) for l, s in zip(lv, single)]
    for m, ls in zip(mods, lv):
        if any(not 0 <= int(f) < m.num_fidelities for f in ls):
            raise ValueError("fidelity %s outside the model's %d levels" % (ls, m.num_fidelities))
    ops = [model_operands(m) for m in mods]
    rnd = [draw_operands(m, nFeatures, generator, o) for m, o in zip(mods, ops)]
    res = ChainDrawResult(names)
    on_device = [i for i, m in enumerate(mods) if engine == "device" and why_not(m) is None]
    if on_device:
        for i, d in zip(on_device, device_draw([ops[i] for i in on_device], [rnd[i] for i in on_device], [lv[i] for i in on_device])):
            res.draws[names[i]] = d
    for i, m in enumerate(mods):
        if i not in on_device:
            dev = m.x_train.device if m.x_train.is_cuda else None
            res.draws[names[i]] = host_draw(ops[i], rnd[i], lv[i], dev)
    for i, k in enumerate(names):
        d = res.draws[k]
        res.engines[k] = d.engine
        res.samples[k] = d.samples[int(lv[i][0])] if single[i] else d.samples
    return res


def sample_chain_from_posterior(model, fidelity, nFeatures=500, generator=None, engine="device"):
    """``MFGP.sample_chain_from_posterior``: one function sample of ``model`` at level ``fidelity`` as an ``RFFChainSample`` with
    one kind-0 layer of 2 nFeatures features."""
    if engine not in ("host", "device"):
        raise ValueError("sample_chain_from_posterior: engine is \"host\" or \"device\" (got %r)" % (engine,))
    if not 0 <= int(fidelity) < model.num_fidelities:
        raise ValueError("fidelity %r outside the model's %d levels" % (fidelity, model.num_fidelities))
    if int(nFeatures) < 1:
        raise ValueError("nFeatures must be >= 1")
    if engine == "device":
        reason = why_not(model)
        if reason is not None:
            raise RuntimeError("sample_chain_from_posterior(engine=\"device\"): " + reason)
    res = draw_chain_samples([model], int(fidelity), nFeatures=nFeatures, generator=generator, engine=engine)
    model.last_draw = res.draws[0]
    return res.samples[0]
