"""torch.autograd wrappers over the C-ABI (device pointers in, device pointers out).

PyTorch is plumbing here: it owns device memory, streams and the autograd tape; all arithmetic of
the layer runs in libmobocmf_hip.so.  Tensors must be CUDA(HIP) float64; there is no CPU fallback.
"""
import contextlib
import ctypes
import os
import threading

import torch

from . import _lib
from ._lib import LayerDesc

JITTER = 1e-6        # gpytorch.settings.variational_cholesky_jitter, float64
MIN_VARIANCE = 1e-10  # gpytorch.settings.min_variance, float64

_scratch = {}


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _prep(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise _lib.MobocmfError("mobocmf_amd: expected a GPU tensor (the HIP path has no CPU fallback)")
    if t.dtype != torch.float64:
        raise _lib.MobocmfError("mobocmf_amd: the hot path is float64 end to end (got %s)" % t.dtype)
    if t.device.index != torch.cuda.current_device():
        # work is enqueued on the CURRENT device's stream: one process per GPU (torch.cuda.set_device first)
        raise _lib.MobocmfError("mobocmf_amd: tensor on %s but the current device is cuda:%d -- call "
                                "torch.cuda.set_device (one process per GPU)" % (t.device, torch.cuda.current_device()))
    return t.contiguous()


_POISON = bool(int(os.environ.get("MOBOCMF_POISON", "0")))   # debugging aid: NaN-fill every workspace before use


def _poison(buf):
    if _POISON and not torch.cuda.is_current_stream_capturing():
        buf[:buf.numel() // 8 * 8].view(torch.float64).fill_(float("nan"))
    return buf


def _empty(*shape, dtype=torch.float64, device=None):
    """Output allocation; NaN-filled under MOBOCMF_POISON so that a kernel leaving part of an output unwritten shows."""
    t = torch.empty(*shape, dtype=dtype, device=device)
    if _POISON and dtype == torch.float64 and not torch.cuda.is_current_stream_capturing():
        t.fill_(float("nan"))
    return t


def _empty_like(t):
    return _empty(t.shape, dtype=t.dtype, device=t.device)


def scratch_buffer(nbytes, device):
    """Per (device, stream) scratch, grown on demand; dead after each C call.  A buffer handed out while the stream is
    being captured is baked into the graph: it is also recorded in ``_capture_pins`` so that the object owning the graph
    can keep it alive (``take_capture_pins``) -- growing the arena later must not free memory a live graph replays on."""
    key = (device.index, torch.cuda.current_stream().cuda_stream)
    buf = _scratch.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(int(nbytes * 1.05) + 4096, dtype=torch.uint8, device=device)
        _scratch[key] = buf
    if torch.cuda.is_current_stream_capturing() and not any(b is buf for b in _capture_pins):
        _capture_pins.append(buf)
    return _poison(buf)


_capture_pins = []


def take_capture_pins():
    """The scratch buffers handed out under capture since the last call (the caller -- a graphed step -- holds them for as
    long as its graph lives)."""
    out = list(_capture_pins)
    _capture_pins.clear()
    return out


def release_scratch(stream=None):
    """Drop the arena's entry of ``stream`` (all entries without an argument): the memory returns to the allocator once
    no graph pins it.  Fitters call this when a training phase's streams retire (torch hands stream handles out of a
    small pool, so a stale entry would otherwise pin up to ~1 GB per handle for ever)."""
    if stream is None:
        _scratch.clear()
        return
    for key in [k for k in _scratch if k[1] == stream.cuda_stream]:
        del _scratch[key]


def hyp_len(kind, d):
    return 1 + d if kind == 0 else 5 + 2 * d


# ---------------------------------------------------------------------------------------------------------------------
# Kernel-selection knobs (include/mobocmf_hip.h: mobocmf_tuning).  The LIBRARY keeps no state: the values travel with every
# call.  This module keeps the host-side default record (`set_*` below change it: size sweeps, A/B timing, parity tests) and a
# per-thread override (`tuning(...)` context manager).  A descriptor takes a SNAPSHOT when it is built in the forward; the
# backward -- which autograd runs on its own thread -- reuses the forward's snapshot, so a call is sized and launched under one
# set of values whatever happens to the defaults in between.
# ---------------------------------------------------------------------------------------------------------------------
_TUNING_DEFAULT = None
_tuning_tls = threading.local()


def _default_tuning():
    global _TUNING_DEFAULT
    if _TUNING_DEFAULT is None:
        t = _lib.Tuning()
        _lib.check(_lib.load().mobocmf_tuning_init(ctypes.byref(t)), "mobocmf_tuning_init")
        _TUNING_DEFAULT = t
    return _TUNING_DEFAULT


def current_tuning():
    """A snapshot (copy) of the tuning calls issued by this thread use now."""
    t = getattr(_tuning_tls, "override", None)
    return (t if t is not None else _default_tuning()).copy()


def _set_default(**kw):
    t = _default_tuning()
    for k, v in kw.items():
        assert k in _lib.Tuning.KNOBS, k
        setattr(t, k, int(v))


@contextlib.contextmanager
def tuning(**kw):
    """Per-THREAD override of the knobs for the calls issued inside the block (forward calls; a backward uses the snapshot
    its forward took): ``with F.tuning(tile_rows=64, sparse_backward=0): ...``."""
    prev = getattr(_tuning_tls, "override", None)
    t = current_tuning()
    for k, v in kw.items():
        if k not in _lib.Tuning.KNOBS:
            raise TypeError("unknown tuning knob %r" % k)
        setattr(t, k, int(v))
    _tuning_tls.override = t
    try:
        yield t
    finally:
        _tuning_tls.override = prev


_probe_tls = threading.local()


@contextlib.contextmanager
def probe_events(table, layer=None):
    """Diagnostic (bench.py per_kernel_instep_ms): the PANEL calls issued by this thread inside the block -- those of layer
    index ``layer`` of a batched-chain forward, or every one if None -- carry ``table`` (a ctypes array of PROBE_EVENTS
    hipEvent_t handles) in their descriptor; the backward of such a call records into the same table."""
    prev = getattr(_probe_tls, "cur", None)
    _probe_tls.cur = (table, layer)
    try:
        yield
    finally:
        _probe_tls.cur = prev


def _probe_for(layer):
    cur = getattr(_probe_tls, "cur", None)
    if cur is None or (cur[1] is not None and layer is not None and cur[1] != layer):
        return None
    return cur[0]


def make_desc(kind, d, M, Np, xdiv=1, branch=0, want_dx=False, jitter=JITTER, min_var=MIN_VARIANCE, tune=None,
              probe=None, params_const=False):
    """``params_const``: the parameters are constants (PANEL calls against a FrozenChain only); ``tune``: a Tuning snapshot to carry (default: the calling thread's current one); ``probe``: a ctypes array of
    PROBE_EVENTS hipEvent_t handles (mobocmf_layer_desc.probe_events) or None."""
    if not 1 <= d <= _lib.MAX_D:
        raise _lib.MobocmfError("mobocmf_amd: a layer takes 1..%d input dimensions (got %d): the Gram kernels keep one "
                                "input row in registers" % (_lib.MAX_D, d))
    if not 1 <= xdiv <= _lib.MAX_XDIV:
        raise _lib.MobocmfError("mobocmf_amd: at most %d samples per input row (num_samples_for_acquisition / "
                                "num_samples_for_training), got %d" % (_lib.MAX_XDIV, xdiv))
    desc = LayerDesc(kind=kind, d=d, M=M, xdiv=xdiv, Np=Np, branch=branch, want_dx=int(want_dx), jitter=jitter,
                     min_var=min_var, params_const=int(params_const), reserved=0)
    snap = tune if tune is not None else current_tuning()
    desc.tuning = ctypes.pointer(snap)
    desc._tune = snap              # keeps the snapshot alive as long as the descriptor
    if probe is not None:
        desc.probe_events = ctypes.cast(probe, ctypes.c_void_p)
        desc._probe = probe
    return desc


def workspace_bytes(desc):
    lib = _lib.load()
    a, b = ctypes.c_size_t(), ctypes.c_size_t()
    _lib.check(lib.mobocmf_layer_workspace_bytes(ctypes.byref(desc), ctypes.byref(a), ctypes.byref(b)),
               "mobocmf_layer_workspace_bytes")
    return a.value, b.value


def _inducing_grad_ws(descs, panel, chain, device):
    """The workspace of a `_z` backward call (the inducing-input gradient's partial sums): a buffer of its own -- the call's
    scratch and chain blocks hold the dK / Gm it reads -- from torch's allocator (no host sync, capturable)."""
    lib = _lib.load()
    total = 0
    for desc in descs:
        a, b = ctypes.c_size_t(), ctypes.c_size_t()
        _lib.check(lib.mobocmf_inducing_grad_workspace_bytes(ctypes.byref(desc), ctypes.byref(a), ctypes.byref(b)),
                   "mobocmf_inducing_grad_workspace_bytes")
        total += (a.value if panel else 0) + (b.value if chain else 0)
    return _poison(torch.empty(total, dtype=torch.uint8, device=device))


class _LayerFn(torch.autograd.Function):
    """(mean, var, kl) of one variational layer; see include/mobocmf_hip.h."""

    @staticmethod
    def forward(ctx, x, f, Zx, zf, hyp, m, L_S, kind, xdiv, branch, jitter, min_var, want_dx, info_out):
        lib = _lib.require_device()
        x, f, Zx, zf, hyp, m, L_S = (_prep(t) for t in (x, f, Zx, zf, hyp, m, L_S))
        d, M = Zx.shape[1], Zx.shape[0]
        nbase = x.shape[0]
        Np = nbase * xdiv
        if kind == 1 and (f is None or f.numel() != Np or zf is None or zf.numel() != M):
            raise _lib.MobocmfError("layer kind 1 needs f (N') and zf (M)")
        if hyp.numel() != hyp_len(kind, d) or m.numel() != M or tuple(L_S.shape) != (M, M) or x.shape[1] != d:
            raise _lib.MobocmfError("shape mismatch in layer forward")
        desc = make_desc(kind, d, M, Np, xdiv, branch, want_dx, jitter, min_var)
        sb, cb = workspace_bytes(desc)
        dev = x.device
        saved = _poison(torch.empty(sb, dtype=torch.uint8, device=dev))
        scratch = scratch_buffer(cb, dev)
        mean = _empty(Np, device=dev)
        var = _empty(Np, device=dev)
        kl = _empty((), device=dev)
        info = info_out if info_out is not None else torch.zeros((), dtype=torch.int32, device=dev)
        rc = lib.mobocmf_layer_forward(ctypes.byref(desc), _ptr(x), _ptr(f), _ptr(Zx), _ptr(zf), _ptr(hyp), _ptr(m),
                                       _ptr(L_S), _ptr(mean), _ptr(var), _ptr(kl), _ptr(info), _ptr(saved), sb,
                                       _ptr(scratch), scratch.numel(), _stream())
        _lib.check(rc, "mobocmf_layer_forward")
        ctx.desc, ctx.sb = desc, sb
        ctx.saved_ws = saved
        ctx.save_for_backward(*[t for t in (x, f, Zx, zf, hyp, m, L_S) if t is not None])
        ctx.has_f = f is not None
        return mean, var, kl

    @staticmethod
    def backward(ctx, g_mean, g_var, g_kl):
        lib = _lib.require_device()
        ts = list(ctx.saved_tensors)
        if ctx.has_f:
            x, f, Zx, zf, hyp, m, L_S = ts
        else:
            x, Zx, hyp, m, L_S = ts
            f = zf = None
        desc = ctx.desc
        dev = x.device
        M, d = Zx.shape
        g_mean, g_var, g_kl = (_prep(t) for t in (g_mean, g_var, g_kl))
        _, cb = workspace_bytes(desc)
        scratch = scratch_buffer(cb, dev)
        new = lambda *s: _empty(*s, device=dev)
        g_f = new(desc.Np) if ctx.has_f else None
        g_zf = new(M) if ctx.has_f else None
        g_hyp, g_m, g_LS = new(hyp.numel()), new(M), new(M, M)
        g_x = new(x.shape[0], d) if desc.want_dx else None
        if ctx.needs_input_grad[2]:      # learnable inducing inputs: the same launches, then the row-side Gram backward
            g_Zx = new(M, d)
            zws = _inducing_grad_ws([desc], True, True, dev)
            rc = lib.mobocmf_layer_backward_z(ctypes.byref(desc), _ptr(x), _ptr(f), _ptr(Zx), _ptr(zf), _ptr(hyp), _ptr(m),
                                              _ptr(L_S), _ptr(g_mean), _ptr(g_var), _ptr(g_kl), _ptr(g_f), _ptr(g_zf),
                                              _ptr(g_hyp), _ptr(g_m), _ptr(g_LS), _ptr(g_x), _ptr(g_Zx), _ptr(ctx.saved_ws),
                                              ctx.sb, _ptr(scratch), scratch.numel(), _ptr(zws), zws.numel(), _stream())
            _lib.check(rc, "mobocmf_layer_backward_z")
            return (g_x, g_f, g_Zx, g_zf, g_hyp, g_m, g_LS, None, None, None, None, None, None, None)
        rc = lib.mobocmf_layer_backward(ctypes.byref(desc), _ptr(x), _ptr(f), _ptr(Zx), _ptr(zf), _ptr(hyp), _ptr(m),
                                        _ptr(L_S), _ptr(g_mean), _ptr(g_var), _ptr(g_kl), _ptr(g_f), _ptr(g_zf),
                                        _ptr(g_hyp), _ptr(g_m), _ptr(g_LS), _ptr(g_x), _ptr(ctx.saved_ws), ctx.sb,
                                        _ptr(scratch), scratch.numel(), _stream())
        _lib.check(rc, "mobocmf_layer_backward")
        return (g_x, g_f, None, g_zf, g_hyp, g_m, g_LS, None, None, None, None, None, None, None)


# ------------------------------------------------------------------------------------------------------------
# All layers of a model in one batch of CHAIN launches (include/mobocmf_hip.h, mobocmf_layers_chain_*): the chain is a
# serial string of latency-bound M x M kernels, the layers' chains do not depend on each other, so one z-batched
# sequence divides its length by the number of layers.  One autograd node carries every layer's chain; the per-layer
# PANEL nodes hang off its ``token``, so autograd runs the batched chain backward after all PANEL backwards.
# ------------------------------------------------------------------------------------------------------------
class ChainBatch:
    """Workspace + bookkeeping shared by ``layers_chain`` and the per-layer ``layer_panel_batched`` calls of one forward."""
    __slots__ = ("n", "kinds", "ds", "M", "branch", "jitters", "min_var", "blocks", "stride", "block_bytes", "infos",
                 "kls", "had_panel", "token", "panel_g", "tune")

    def chain_desc(self, z):
        return make_desc(self.kinds[z], self.ds[z], self.M, 1, 1, self.branch, False, self.jitters[z], self.min_var,
                         tune=self.tune)

    def panel_desc(self, z, Np, xdiv, want_dx):
        return make_desc(self.kinds[z], self.ds[z], self.M, Np, xdiv, self.branch, want_dx, self.jitters[z], self.min_var,
                         tune=self.tune, probe=_probe_for(z))

    def block(self, z):
        return self.blocks[z * self.stride:z * self.stride + self.block_bytes]


def _table(ptrs):
    return (ctypes.c_void_p * len(ptrs))(*ptrs)


def _desc_table(descs):
    return (ctypes.POINTER(LayerDesc) * len(descs))(*[ctypes.pointer(d) for d in descs])


class _ChainsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, CB, *flat):
        lib = _lib.require_device()
        n = CB.n
        per = [[_prep(t) for t in flat[5 * z:5 * z + 5]] for z in range(n)]      # Zx, zf, hyp, m, L_S per layer
        dev = per[0][0].device
        descs = [CB.chain_desc(z) for z in range(n)]
        bb, st = ctypes.c_size_t(), ctypes.c_size_t()
        _lib.check(lib.mobocmf_chain_block_bytes(ctypes.byref(descs[0]), ctypes.byref(bb), ctypes.byref(st)),
                   "mobocmf_chain_block_bytes")
        CB.block_bytes = bb.value
        CB.stride = (bb.value + 255) // 256 * 256
        CB.blocks = _poison(torch.empty(n * CB.stride, dtype=torch.uint8, device=dev))
        CB.kls = [_empty((), device=dev) for _ in range(n)]
        CB.had_panel = [0] * n
        CB.panel_g = [None] * n
        ctx.set_materialize_grads(False)
        token = torch.empty(1, dtype=torch.float64, device=dev)      # never read: it only orders the autograd nodes
        P = lambda i, none_ok=False: _table([0 if per[z][i] is None else per[z][i].data_ptr() for z in range(n)])
        rc = lib.mobocmf_layers_chain_forward(n, _desc_table(descs), P(0), P(1), P(2), P(3), P(4),
                                              _table([k.data_ptr() for k in CB.kls]),
                                              _table([t.data_ptr() for t in CB.infos]), _ptr(CB.blocks), CB.stride,
                                              CB.blocks.numel(), _stream())
        _lib.check(rc, "mobocmf_layers_chain_forward")
        ctx.CB = CB
        ctx.descs = descs
        # zf of layer z is the variational mean of layer z - 1 (the model's Z~_z = [Z_x, m_{z-1}]): its gradient is folded into
        # g_m[z - 1] inside the chain backward (had_panel |= 4) instead of by an autograd add of two M-vectors
        same = lambda a, b: a is not None and b is not None and (a is b or (a.data_ptr() == b.data_ptr() and a.shape == b.shape
                                                                            and a.stride() == b.stride()))
        ctx.fold = [z > 0 and CB.kinds[z] == 1 and same(flat[5 * z + 1], flat[5 * (z - 1) + 3]) and
                    bool(ctx.needs_input_grad[1 + 5 * z + 1]) and bool(ctx.needs_input_grad[1 + 5 * (z - 1) + 3])
                    for z in range(n)]
        ctx.has = [[t is not None for t in per[z]] for z in range(n)]
        ctx.save_for_backward(*[t for z in range(n) for t in per[z] if t is not None])
        return (token,) + tuple(CB.kls)

    @staticmethod
    def backward(ctx, g_token, *g_kls):
        lib = _lib.require_device()
        CB = ctx.CB
        n = CB.n
        it = iter(ctx.saved_tensors)
        per = [[next(it) if h else None for h in ctx.has[z]] for z in range(n)]
        dev = per[0][0].device
        gk = [_prep(g) if g is not None else torch.zeros((), dtype=torch.float64, device=dev) for g in g_kls]
        new = lambda *s: _empty(*s, device=dev)
        # a layer whose PANEL half ran left its share of g_hyp / g_zf in CB.panel_g: the chain accumulates into those buffers
        # (had_panel = 2) instead of autograd adding two tensors per layer afterwards
        had = list(CB.had_panel)
        g_zf, g_hyp = [], []
        for z in range(n):
            pg = CB.panel_g[z]
            if pg is not None:
                had[z] = 2
                g_hyp.append(pg[0])
                g_zf.append(pg[1] if per[z][1] is not None else None)
            else:
                g_hyp.append(new(per[z][2].numel()))
                g_zf.append(new(CB.M) if per[z][1] is not None else None)
        g_m = [new(CB.M) for _ in range(n)]
        g_LS = [new(CB.M, CB.M) for _ in range(n)]
        for z in range(n):
            if ctx.fold[z]:
                had[z] |= 4
        T = lambda ts: _table([0 if t is None else t.data_ptr() for t in ts])
        g_Zx = [None] * n
        if any(ctx.needs_input_grad[1 + 5 * z] for z in range(n)):      # learnable inducing inputs: the K_mm shares
            g_Zx = [new(CB.M, CB.ds[z]) for z in range(n)]
            zws = _inducing_grad_ws(ctx.descs, False, True, dev)
            rc = lib.mobocmf_layers_chain_backward_z(n, _desc_table(ctx.descs), T([p[0] for p in per]), T([p[1] for p in per]),
                                                     T([p[2] for p in per]), T(gk), (ctypes.c_int32 * n)(*had),
                                                     T(g_zf), T(g_hyp), T(g_m), T(g_LS), T(g_Zx), _ptr(CB.blocks), CB.stride,
                                                     CB.blocks.numel(), _ptr(zws), zws.numel(), _stream())
            _lib.check(rc, "mobocmf_layers_chain_backward_z")
        else:
            rc = lib.mobocmf_layers_chain_backward(n, _desc_table(ctx.descs), T([p[0] for p in per]), T([p[1] for p in per]),
                                                   T([p[2] for p in per]), T(gk), (ctypes.c_int32 * n)(*had),
                                                   T(g_zf), T(g_hyp), T(g_m), T(g_LS), _ptr(CB.blocks), CB.stride,
                                                   CB.blocks.numel(), _stream())
            _lib.check(rc, "mobocmf_layers_chain_backward")
        out = [None]
        for z in range(n):
            out += [g_Zx[z] if ctx.needs_input_grad[1 + 5 * z] else None, None if ctx.fold[z] else g_zf[z], g_hyp[z], g_m[z],
                    g_LS[z]]
        return tuple(out)


def layers_chain(layers_params, kinds, branch, jitters, infos, min_var=MIN_VARIANCE):
    """CHAIN halves of all layers in one batch.  ``layers_params``: per layer (Zx, zf or None, hyp, m, L_S), equal M.
    Returns the ChainBatch (``.kls`` = per-layer KL tensors with gradient, ``.token`` for the PANEL calls)."""
    CB = ChainBatch()
    CB.n = len(layers_params)
    if not 1 <= CB.n <= 4:
        raise _lib.MobocmfError("layers_chain: 1..4 layers per batch")
    CB.kinds, CB.ds = list(kinds), [p[0].shape[1] for p in layers_params]
    CB.M = layers_params[0][0].shape[0]
    if any(p[0].shape[0] != CB.M for p in layers_params):
        raise _lib.MobocmfError("layers_chain: the layers must share the number of inducing points")
    CB.branch, CB.jitters, CB.min_var, CB.infos = branch, list(jitters), min_var, list(infos)
    CB.tune = current_tuning()      # one snapshot for the chains and every PANEL call that hangs off them
    out = _ChainsFn.apply(CB, *[t for p in layers_params for t in p])
    CB.token, CB.kls = out[0], list(out[1:])
    return CB


class _PanelBatchedFn(torch.autograd.Function):
    """The PANEL half of one layer against its chain: slot ``z`` of a ChainBatch, or a FrozenChain (``token`` None, ``z`` not
    used) -- then the chain state is only read and the gradients stop at x and f."""

    @staticmethod
    def forward(ctx, x, f, Zx, zf, hyp, token, CB, z, xdiv, want_dx):
        lib = _lib.require_device()
        x, f, Zx, zf, hyp = (_prep(t) for t in (x, f, Zx, zf, hyp))
        Np = x.shape[0] * xdiv
        desc = CB.panel_desc(z, Np, xdiv, want_dx)
        if x.shape[1] != desc.d or (desc.kind == 1 and (f is None or f.numel() != Np)):
            raise _lib.MobocmfError("shape mismatch between the chain and a panel call")
        dev = x.device
        sb, cb = ctypes.c_size_t(), ctypes.c_size_t()
        _lib.check(lib.mobocmf_panel_workspace_bytes(ctypes.byref(desc), ctypes.byref(sb), ctypes.byref(cb)),
                   "mobocmf_panel_workspace_bytes")
        saved = _poison(torch.empty(sb.value, dtype=torch.uint8, device=dev))
        scratch = scratch_buffer(cb.value, dev)
        mean, var = _empty(Np, device=dev), _empty(Np, device=dev)
        blk = CB.block(z)
        rc = lib.mobocmf_layer_panel_forward(ctypes.byref(desc), _ptr(x), _ptr(f), _ptr(Zx), _ptr(zf), _ptr(hyp),
                                             _ptr(mean), _ptr(var), _ptr(blk), blk.numel(), _ptr(saved), sb.value,
                                             _ptr(scratch), scratch.numel(), _stream())
        _lib.check(rc, "mobocmf_layer_panel_forward")
        ctx.CB, ctx.z, ctx.desc, ctx.saved_ws, ctx.sb, ctx.cb = CB, z, desc, saved, sb.value, cb.value
        ctx.save_for_backward(*[t for t in (x, f, Zx, zf, hyp) if t is not None])
        ctx.has_f = f is not None
        return mean, var

    @staticmethod
    def backward(ctx, g_mean, g_var):
        lib = _lib.require_device()
        CB, z, desc = ctx.CB, ctx.z, ctx.desc
        ts = list(ctx.saved_tensors)
        if ctx.has_f:
            x, f, Zx, zf, hyp = ts
        else:
            x, Zx, hyp = ts
            f = zf = None
        dev = x.device
        g_mean, g_var = _prep(g_mean), _prep(g_var)
        scratch = scratch_buffer(ctx.cb, dev)      # H / Hc / da (if any) go to the chain block, nothing of the scratch is kept
        new = lambda *s: _empty(*s, device=dev)
        g_f = new(desc.Np) if ctx.has_f else None
        g_zf = new(CB.M) if ctx.has_f else None
        g_hyp = new(hyp.numel())
        g_x = new(x.shape[0], desc.d) if desc.want_dx else None
        blk = CB.block(z)
        g_Zx = None
        if ctx.needs_input_grad[2] and not desc.params_const:      # learnable inducing inputs: the K_mn share
            g_Zx = new(CB.M, desc.d)
            zws = _inducing_grad_ws([desc], True, False, dev)
            rc = lib.mobocmf_layer_panel_backward_z(ctypes.byref(desc), _ptr(x), _ptr(f), _ptr(Zx), _ptr(zf), _ptr(hyp),
                                                    _ptr(g_mean), _ptr(g_var), _ptr(g_f), _ptr(g_zf), _ptr(g_hyp), _ptr(g_x),
                                                    _ptr(g_Zx), _ptr(blk), blk.numel(), _ptr(ctx.saved_ws), ctx.sb,
                                                    _ptr(scratch), scratch.numel(), _ptr(zws), zws.numel(), _stream())
            _lib.check(rc, "mobocmf_layer_panel_backward_z")
        else:
            rc = lib.mobocmf_layer_panel_backward(ctypes.byref(desc), _ptr(x), _ptr(f), _ptr(Zx), _ptr(zf), _ptr(hyp),
                                                  _ptr(g_mean), _ptr(g_var), _ptr(g_f), _ptr(g_zf), _ptr(g_hyp), _ptr(g_x),
                                                  _ptr(blk), blk.numel(), _ptr(ctx.saved_ws), ctx.sb, _ptr(scratch),
                                                  scratch.numel(), _stream())
            _lib.check(rc, "mobocmf_layer_panel_backward")
        if desc.params_const:
            return g_x, g_f, None, None, None, None, None, None, None, None
        CB.had_panel[z] = 1
        # the K_mn share of g_hyp / g_zf is handed to the chain node (which adds its K_mm share into the same buffers), and
        # None for the token: the edge to the chain node orders the backward passes, no gradient has to flow through it
        CB.panel_g[z] = (g_hyp, g_zf)
        return g_x, g_f, g_Zx, None, None, None, None, None, None, None


def layer_panel_batched(CB, z, x, f, Zx, zf, hyp, xdiv=1, want_dx=False):
    """PANEL half of layer ``z`` of a chain batch: mean (N'), var (N')."""
    return _PanelBatchedFn.apply(x, f, Zx, zf, hyp, CB.token, CB, z, xdiv, want_dx)


class FrozenChain:
    """CHAIN state of one layer for FIXED parameters (acquisition optimisation): computed once, then read in place by every
    PANEL call (any number of them, on any stream); gradients flow to the layer inputs only."""
    __slots__ = ("kind", "d", "M", "branch", "jitter", "min_var", "state", "kl", "info", "Zx", "zf", "hyp")

    def panel_desc(self, z, Np, xdiv, want_dx):
        return make_desc(self.kind, self.d, self.M, Np, xdiv, self.branch, want_dx, self.jitter, self.min_var,
                         probe=_probe_for(None), params_const=True)

    def block(self, z):
        return self.state


def freeze_chain(Zx, zf, hyp, m, L_S, kind, branch=1, jitter=JITTER, min_var=MIN_VARIANCE):
    """The FrozenChain of one layer: a one-layer chain batch into a temporary block, of which the state is kept."""
    lib = _lib.require_device()
    with torch.no_grad():
        Zx, zf, hyp, m, L_S = (_prep(None if t is None else t.detach()) for t in (Zx, zf, hyp, m, L_S))
        fc = FrozenChain()
        fc.kind, fc.d, fc.M, fc.branch, fc.jitter, fc.min_var = kind, Zx.shape[1], Zx.shape[0], branch, jitter, min_var
        fc.Zx, fc.zf, fc.hyp = Zx, zf, hyp
        dev = Zx.device
        desc = make_desc(kind, fc.d, fc.M, 1, 1, branch, False, jitter, min_var)
        bb, st = ctypes.c_size_t(), ctypes.c_size_t()
        _lib.check(lib.mobocmf_chain_block_bytes(ctypes.byref(desc), ctypes.byref(bb), ctypes.byref(st)),
                   "mobocmf_chain_block_bytes")
        stride = (bb.value + 255) // 256 * 256
        block = _poison(torch.empty(stride, dtype=torch.uint8, device=dev))
        fc.kl = _empty((), device=dev)
        fc.info = torch.zeros((), dtype=torch.int32, device=dev)
        T = lambda t: _table([0 if t is None else t.data_ptr()])
        rc = lib.mobocmf_layers_chain_forward(1, _desc_table([desc]), T(Zx), T(zf), T(hyp), T(m), T(L_S), T(fc.kl), T(fc.info),
                                              _ptr(block), stride, block.numel(), _stream())
        _lib.check(rc, "mobocmf_layers_chain_forward")
        fc.state = block[:st.value].clone()
    return fc


def layer_panel_frozen(fc, x, f, xdiv=1, want_dx=False):
    """mean (N'), var (N') against a FrozenChain; differentiable w.r.t. f (and x if want_dx) only."""
    return _PanelBatchedFn.apply(x, f, fc.Zx, fc.zf, fc.hyp, None, fc, 0, xdiv, want_dx)


def layer_forward(x, f, Zx, zf, hyp, m, L_S, kind, xdiv=1, branch=0, jitter=JITTER, min_var=MIN_VARIANCE,
                  want_dx=False, info_out=None):
    """mean (N'), var (N'), kl ()  --  N' = x.shape[0] * xdiv."""
    return _LayerFn.apply(x, f, Zx, zf, hyp, m, L_S, kind, xdiv, branch, jitter, min_var, want_dx, info_out)


def predictive_covariance(x, f, Zx, zf, hyp, m, L_S, kind, xdiv=1, jitter=JITTER, chain=None):
    """Full eval-branch predictive covariance (N' x N') -- K10: symmetric rank-M updates on the MFMA, lower tiles only,
    any N'.  Returns (mean, cov).  ``chain``: a FrozenChain of the same layer (then m, L_S are not needed and the M x M
    chain is not recomputed).  No autograd."""
    lib = _lib.require_device()
    with torch.no_grad():
        x, f, Zx, zf, hyp, m, L_S = (_prep(t) for t in (x, f, Zx, zf, hyp, m, L_S))
        d, M = Zx.shape[1], Zx.shape[0]
        Np = x.shape[0] * xdiv
        dev = x.device
        if chain is None:
            chain = freeze_chain(Zx, zf, hyp, m, L_S, kind, branch=1, jitter=jitter)
        desc = make_desc(kind, d, M, Np, xdiv, 1, False, jitter, MIN_VARIANCE)
        mean, _ = layer_panel_frozen(chain, x, f, xdiv=xdiv)
        cb = ctypes.c_size_t()
        _lib.check(lib.mobocmf_predictive_covariance_workspace_bytes(ctypes.byref(desc), ctypes.byref(cb)),
                   "mobocmf_predictive_covariance_workspace_bytes")
        scratch = scratch_buffer(cb.value, dev)
        cov = _empty(Np, Np, device=dev)
        _lib.check(lib.mobocmf_predictive_covariance(ctypes.byref(desc), _ptr(x), _ptr(f), _ptr(Zx), _ptr(zf), _ptr(hyp),
                                                     _ptr(cov), Np, _ptr(chain.state), chain.state.numel(), _ptr(scratch),
                                                     scratch.numel(), _stream()), "mobocmf_predictive_covariance")
    return mean, cov


def _propagate_backward(ctx, g, add_mean=None, add_var=None):
    """g_mean / g_var of the previous layer's moments: zeros beyond the propagated prefix (one launch either way).
    add_mean / add_var: the gradients the pass-through copies of the moments received (``through=True``), added in the same
    launch."""
    lib = _lib.require_device()
    var, eps = ctx.saved_tensors
    if g is None:        # nothing came back through the propagated samples
        if add_mean is None and add_var is None:
            return None, None
        z = lambda t: _prep(t) if t is not None else torch.zeros_like(var)
        return z(add_mean), z(add_var)
    g = _prep(g)
    add_mean = None if add_mean is None else _prep(add_mean.reshape(-1))
    add_var = None if add_var is None else _prep(add_var.reshape(-1))
    gm, gv = _empty_like(var), _empty_like(var)
    _lib.check(lib.mobocmf_propagate_backward_prefix(_ptr(var), _ptr(eps), _ptr(g), _ptr(gm), _ptr(gv), eps.numel(),
                                                     ctx.div, var.numel(), _ptr(add_mean), _ptr(add_var), _stream()),
               "mobocmf_propagate_backward_prefix")
    return gm, gv


class _PropagateFn(torch.autograd.Function):
    """f~ = mean + sqrt(var) eps.  through=True additionally returns pass-through aliases of (mean, var): a caller that
    also scores the SAME moments (the ELBO's data term of the previous layer's own fidelity) uses those, so the moments have
    one consumer node and their two gradient contributions are summed inside the propagate-backward launch."""

    @staticmethod
    def forward(ctx, mean, var, eps, div, through):
        lib = _lib.require_device()
        shape = mean.shape
        mean, var, eps = _prep(mean.reshape(-1)), _prep(var.reshape(-1)), _prep(eps.reshape(-1))
        n = eps.numel()
        if mean.numel() * div < n or n % div or var.numel() != mean.numel():
            raise _lib.MobocmfError("propagate: eps must have k*div entries, k <= mean.numel() (a prefix of the rows)")
        out = _empty(n, device=mean.device)
        _lib.check(lib.mobocmf_propagate_forward(_ptr(mean), _ptr(var), _ptr(eps), _ptr(out), n, div, _stream()),
                   "mobocmf_propagate_forward")
        ctx.save_for_backward(var, eps)
        ctx.div, ctx.shape = div, shape
        ctx.set_materialize_grads(False)
        if through:
            return out, mean.view(shape), var.view(shape)
        return out

    @staticmethod
    def backward(ctx, g, g_mean_t=None, g_var_t=None):
        gm, gv = _propagate_backward(ctx, g, g_mean_t, g_var_t)
        r = lambda t: None if t is None else t.view(ctx.shape)
        return r(gm), r(gv), None, None, None


class _PropagateRngFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mean, var, rng_state, n_out, div, through):
        lib = _lib.require_device()
        shape = mean.shape
        mean, var = _prep(mean.reshape(-1)), _prep(var.reshape(-1))
        if mean.numel() * div < n_out or n_out % div or var.numel() != mean.numel() or rng_state.dtype != torch.int64 or \
                rng_state.numel() != 3 or not rng_state.is_cuda:
            raise _lib.MobocmfError("propagate_rng: n_out must be k*div, k <= mean.numel(), and rng_state three int64 on the GPU")
        out, eps = _empty(n_out, device=mean.device), _empty(n_out, device=mean.device)
        _lib.check(lib.mobocmf_propagate_rng_forward(_ptr(mean), _ptr(var), _ptr(rng_state), _ptr(out), _ptr(eps), n_out, div,
                                                     _stream()), "mobocmf_propagate_rng_forward")
        ctx.save_for_backward(var, eps)
        ctx.div, ctx.shape = div, shape
        ctx.mark_non_differentiable(eps)
        ctx.set_materialize_grads(False)      # no zero-filled "gradient of eps" (a fill launch per backward)
        if through:
            return out, eps, mean.view(shape), var.view(shape)
        return out, eps

    @staticmethod
    def backward(ctx, g, _g_eps, g_mean_t=None, g_var_t=None):
        gm, gv = _propagate_backward(ctx, g, g_mean_t, g_var_t)
        r = lambda t: None if t is None else t.view(ctx.shape)
        return r(gm), r(gv), None, None, None, None


def propagate_rng(mean, var, rng_state, n_out, div=1):
    """f~[n] = mean[n/div] + sqrt(var[n/div]) * eps[n] with eps ~ N(0, 1) drawn inside the launch (Philox4x32-10 keyed by
    rng_state = int64 [seed, calls, ticket] on the device; every call advances ``calls``).  Returns (f~, eps)."""
    return _PropagateRngFn.apply(mean, var, rng_state, int(n_out), int(div), False)


def propagate_rng_through(mean, var, rng_state, n_out, div=1):
    """``propagate_rng`` + pass-through aliases: returns (f~, eps, mean', var'); score mean' / var' instead of mean / var."""
    return _PropagateRngFn.apply(mean, var, rng_state, int(n_out), int(div), True)


def propagate(mean, var, eps, div=1):
    """f~[n] = mean[n/div] + sqrt(var[n/div]) * eps[n]   (mfdgp_hidden_layer.py:263-274).  ``eps`` may cover only a prefix of
    the rows of (mean, var): the rest is not propagated and gets zero gradient."""
    return _PropagateFn.apply(mean, var, eps, div, False)


def propagate_through(mean, var, eps, div=1):
    """``propagate`` + pass-through aliases: returns (f~, mean', var'); score mean' / var' instead of mean / var."""
    return _PropagateFn.apply(mean, var, eps, div, True)


class _ElboDataFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mean, var, y, fid, tau, level, div, lo=0.0, hi=0.0):
        lib = _lib.require_device()
        mean, var, y, fid, tau = (_prep(t.reshape(-1)) for t in (mean, var, y, fid, tau))
        n = mean.numel()
        if y.numel() * div != n or fid.numel() != y.numel():
            raise _lib.MobocmfError("elbo_data: shape mismatch")
        out = _empty((), device=mean.device)
        scratch = scratch_buffer(8192, mean.device)
        _lib.check(lib.mobocmf_elbo_data_interval_forward(_ptr(mean), _ptr(var), _ptr(y), _ptr(fid), _ptr(tau), float(lo),
                                                          float(hi), float(level), n, div, _ptr(out), _ptr(scratch),
                                                          scratch.numel(), _stream()),
                   "mobocmf_elbo_data_forward")
        ctx.save_for_backward(mean, var, y, fid, tau)
        ctx.level, ctx.div, ctx.lo, ctx.hi = float(level), div, float(lo), float(hi)
        return out

    @staticmethod
    def backward(ctx, g):
        lib = _lib.require_device()
        mean, var, y, fid, tau = ctx.saved_tensors
        g = _prep(g)
        gm, gv = _empty_like(mean), _empty_like(var)
        gt = _empty_like(tau)
        scratch = scratch_buffer(8192, mean.device)
        _lib.check(lib.mobocmf_elbo_data_interval_backward(_ptr(mean), _ptr(var), _ptr(y), _ptr(fid), _ptr(tau), ctx.lo,
                                                           ctx.hi, ctx.level, mean.numel(), ctx.div, _ptr(g), _ptr(gm),
                                                           _ptr(gv), _ptr(gt), _ptr(scratch), scratch.numel(), _stream()),
                   "mobocmf_elbo_data_backward")
        return gm, gv, None, None, gt.reshape(ctx.saved_tensors[4].shape), None, None, None, None


def elbo_data(mean, var, y, fid, tau, level, div=1, interval=None):
    """(1/div) sum_{fid==level} E_q[log N(y | f, tau)]   (variational_elbo_mf.py:31-35).
    ``interval=(lo, hi)``: ``tau`` is the RAW noise parameter of an Interval constraint; the sigmoid transform and its
    chain rule run inside the kernels (six element-wise launches less per fidelity and step)."""
    if interval is not None:
        return _ElboDataFn.apply(mean, var, y, fid, tau, level, div, float(interval[0]), float(interval[1]))
    return _ElboDataFn.apply(mean, var, y, fid, tau, level, div)


class _ShortcutVarFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, L_S, min_var):
        lib = _lib.require_device()
        L_S = _prep(L_S)
        M = L_S.shape[0]
        var = _empty(M, device=L_S.device)
        _lib.check(lib.mobocmf_shortcut_var_forward(_ptr(L_S), M, float(min_var), _ptr(var), _stream()),
                   "mobocmf_shortcut_var_forward")
        ctx.save_for_backward(L_S, var)
        ctx.min_var = float(min_var)
        return var

    @staticmethod
    def backward(ctx, g):
        lib = _lib.require_device()
        L_S, var = ctx.saved_tensors
        g = _prep(g)
        gL = _empty_like(L_S)
        _lib.check(lib.mobocmf_shortcut_var_backward(_ptr(L_S), _ptr(var), _ptr(g), L_S.shape[0], ctx.min_var, _ptr(gL),
                                                     _stream()), "mobocmf_shortcut_var_backward")
        return gL, None


def shortcut_var(L_S, min_var=MIN_VARIANCE):
    """diag(L_S L_S^T) floored at min_var: the marginal variances of q(u) (GPyTorch's equal-inputs shortcut)."""
    return _ShortcutVarFn.apply(L_S, min_var)


class _ElboCombineFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scale, n_data, *terms):
        lib = _lib.require_device()
        terms = [_prep(t.reshape(())) for t in terms]
        data, kls = terms[:n_data], terms[n_data:]
        out = _empty(2, device=terms[0].device)
        A = (ctypes.c_void_p * max(len(data), 1))(*[t.data_ptr() for t in data])
        B = (ctypes.c_void_p * max(len(kls), 1))(*[t.data_ptr() for t in kls])
        _lib.check(lib.mobocmf_elbo_combine_forward(len(data), A, len(kls), B, float(scale), _ptr(out), _stream()),
                   "mobocmf_elbo_combine_forward")
        ctx.scale, ctx.n_data, ctx.n = float(scale), n_data, len(terms)
        ctx.keep = terms               # the table holds raw pointers: keep the scalars alive until the launch is enqueued
        return out[0], out[1]

    @staticmethod
    def backward(ctx, g_elbo, g_skl):
        lib = _lib.require_device()
        ref = g_elbo if g_elbo is not None else g_skl
        g = _empty(2, device=ref.device)
        ge = None if g_elbo is None else _prep(g_elbo)
        gs = None if g_skl is None else _prep(g_skl)
        _lib.check(lib.mobocmf_elbo_combine_backward(_ptr(ge), _ptr(gs), ctx.scale, _ptr(g), _stream()),
                   "mobocmf_elbo_combine_backward")
        return (None, None) + (g[0],) * ctx.n_data + (g[1],) * (ctx.n - ctx.n_data)


def elbo_combine(data_terms, kls, scale):
    """(sum data - scale * sum kl, scale * sum kl) in one launch (and one in backward)."""
    if len(data_terms) > 8 or len(kls) > 8:
        d = sum(data_terms) if data_terms else 0.0
        k = sum(kls) * scale if kls else 0.0
        return d - k, k
    return _ElboCombineFn.apply(scale, len(data_terms), *data_terms, *kls)


class _ElboFusedFn(torch.autograd.Function):
    """(elbo, scaled_kl, -elbo) of variational_elbo_mf.py:24-51 in one launch, one more in backward (mobocmf_elbo_forward)."""

    @staticmethod
    def forward(ctx, scale, B, specs, y, fid, n_kl, *tensors):
        # specs[l] = None | (div, lo, hi, rows): the layer holds the first ``rows`` base rows of the batch
        lib = _lib.require_device()
        L = len(specs)
        y, fid = _prep(y.reshape(-1)), _prep(fid.reshape(-1))
        dev = y.device
        means, vars_, raws, it = [None] * L, [None] * L, [None] * L, iter(tensors)
        for l, sp in enumerate(specs):
            if sp is not None:
                means[l], vars_[l], raws[l] = _prep(next(it).reshape(-1)), _prep(next(it).reshape(-1)), _prep(next(it).reshape(-1))
                if means[l].numel() != sp[3] * sp[0] or vars_[l].numel() != sp[3] * sp[0] or not 0 <= sp[3] <= B:
                    raise _lib.MobocmfError("elbo: layer %d holds %d rows, expected %d" % (l, means[l].numel(), sp[3] * sp[0]))
        kls = [_prep(next(it).reshape(())) for _ in range(n_kl)]
        if y.numel() != B or fid.numel() != B:
            raise _lib.MobocmfError("elbo: target / fidelities shape mismatch")
        out = _empty(3, device=dev)
        scratch = scratch_buffer(8 * 512 * 8, dev)
        T = lambda ts: _table([0 if t is None else t.data_ptr() for t in ts])
        div = (ctypes.c_int32 * L)(*[1 if sp is None else sp[0] for sp in specs])
        lo = (ctypes.c_double * L)(*[0.0 if sp is None else sp[1] for sp in specs])
        hi = (ctypes.c_double * L)(*[0.0 if sp is None else sp[2] for sp in specs])
        rows = (ctypes.c_int64 * L)(*[B if sp is None else sp[3] for sp in specs])
        _lib.check(lib.mobocmf_elbo_forward(L, T(means), T(vars_), div, T(raws), lo, hi, _ptr(y), _ptr(fid), B, rows, n_kl,
                                            T(kls) if n_kl else None, float(scale), _ptr(out), _ptr(scratch),
                                            scratch.numel(), _stream()), "mobocmf_elbo_forward")
        ctx.set_materialize_grads(False)
        ctx.meta = (float(scale), B, specs, n_kl, [None if t is None else t.shape for t in tensors])
        ctx.save_for_backward(y, fid, *[t for l in range(L) if specs[l] is not None for t in (means[l], vars_[l], raws[l])])
        elbo, skl, neg = out[0], out[1], out[2]
        ctx.mark_non_differentiable(neg)
        return elbo, skl, neg

    @staticmethod
    def backward(ctx, g_elbo, g_skl, _g_neg):
        lib = _lib.require_device()
        scale, B, specs, n_kl, shapes = ctx.meta
        L = len(specs)
        y, fid = ctx.saved_tensors[:2]
        it = iter(ctx.saved_tensors[2:])
        dev = y.device
        means, vars_, raws = [None] * L, [None] * L, [None] * L
        gm, gv, gr = [None] * L, [None] * L, [None] * L
        for l, sp in enumerate(specs):
            if sp is not None:
                means[l], vars_[l], raws[l] = next(it), next(it), next(it)
                gm[l], gv[l], gr[l] = _empty_like(means[l]), _empty_like(vars_[l]), _empty_like(raws[l])
                if means[l].numel() == 0:      # a layer of no rows has no storage: the kernel sees it as absent and writes nothing
                    gr[l].zero_()
        gkl = _empty(1, device=dev)
        ge = None if g_elbo is None else _prep(g_elbo)
        gs = None if g_skl is None else _prep(g_skl)
        scratch = scratch_buffer(8 * 512 * 8, dev)
        T = lambda ts: _table([0 if t is None else t.data_ptr() for t in ts])
        div = (ctypes.c_int32 * L)(*[1 if sp is None else sp[0] for sp in specs])
        lo = (ctypes.c_double * L)(*[0.0 if sp is None else sp[1] for sp in specs])
        hi = (ctypes.c_double * L)(*[0.0 if sp is None else sp[2] for sp in specs])
        rows = (ctypes.c_int64 * L)(*[B if sp is None else sp[3] for sp in specs])
        _lib.check(lib.mobocmf_elbo_backward(L, T(means), T(vars_), div, T(raws), lo, hi, _ptr(y), _ptr(fid), B, rows, scale,
                                             _ptr(ge), _ptr(gs), T(gm), T(gv), T(gr), _ptr(gkl), _ptr(scratch),
                                             scratch.numel(), _stream()), "mobocmf_elbo_backward")
        grads, k = [], 0
        for l, sp in enumerate(specs):
            if sp is not None:
                grads += [gm[l].reshape(shapes[k]), gv[l].reshape(shapes[k + 1]), gr[l].reshape(shapes[k + 2])]
                k += 3
        grads += [gkl[0]] * n_kl
        return (None,) * 6 + tuple(grads)


ELBO_MAX_LAYERS = 8


def elbo_fused(layers, y, fid, kls, scale):
    """``layers``: per fidelity level None or (mean, var, raw_noise, div, lo, hi[, rows]) -- hi <= lo: ``raw_noise`` is the
    noise itself; ``rows`` (default: all of y): the layer holds the first ``rows`` rows of the batch only (rows * div
    entries).  Returns (elbo, scaled_kl, -elbo); the last one carries no gradient (the loss value a training step reports)."""
    B = int(y.numel())
    specs = [None if lay is None else (int(lay[3]), float(lay[4]), float(lay[5]), int(lay[6]) if len(lay) > 6 else B)
             for lay in layers]
    tensors = [t for lay in layers if lay is not None for t in lay[:3]]
    return _ElboFusedFn.apply(float(scale), int(y.numel()), specs, y, fid, len(kls), *tensors, *kls)


# ---------------------------------------------------------------------------------------------------------------------
# Conditioned training: the theta / omega factor losses and the glue around them, one launch each way
# (include/mobocmf_hip.h: mobocmf_cond_factors_forward, _scale_segments, _gather_segments, _scalar_combine).
# ---------------------------------------------------------------------------------------------------------------------
def _ptr_table(ts):
    return (ctypes.c_void_p * max(len(ts), 1))(*[0 if t is None else t.data_ptr() for t in ts])


class _SplitRowsFn(torch.autograd.Function):
    """(mean, var) -> their consecutive row ranges [0, c0), [c0, c0 + c1), ... as views (no launch); the backward writes the
    ranges' gradients -- zeros where a range got none -- into one buffer in ONE launch (autograd's slice backward: a zero fill,
    a copy and an add per range and tensor)."""

    @staticmethod
    def forward(ctx, mean, var, *counts):
        ctx.shapes = (mean.shape, var.shape)
        mean, var = _prep(mean.reshape(-1)), _prep(var.reshape(-1))
        if sum(counts) != mean.numel() or var.numel() != mean.numel():
            raise _lib.MobocmfError("split_rows: the counts must add up to the number of rows")
        ctx.counts = tuple(int(c) for c in counts)
        ctx.set_materialize_grads(False)
        outs, off = [], 0
        for t in (mean, var):
            off = 0
            for c in ctx.counts:
                outs.append(t[off:off + c])
                off += c
        ctx.dev = mean.device
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gs):
        lib = _lib.require_device()
        k, n = len(ctx.counts), sum(ctx.counts)
        if all(g is None for g in gs):
            return (None, None) + (None,) * k
        gs = [None if g is None else _prep(g.reshape(-1)) for g in gs]
        out = _empty(2 * n, device=ctx.dev)
        sizes = (ctypes.c_int64 * (2 * k))(*(list(ctx.counts) * 2))
        _lib.check(lib.mobocmf_gather_segments(2 * k, _ptr_table(gs), sizes, _ptr(out), _stream()), "mobocmf_gather_segments")
        return (out[:n].view(ctx.shapes[0]), out[n:].view(ctx.shapes[1])) + (None,) * k


def split_rows(mean, var, counts):
    """Consecutive row ranges of (mean, var): returns ([mean ranges], [var ranges])."""
    outs = _SplitRowsFn.apply(mean, var, *counts)
    k = len(counts)
    return list(outs[:k]), list(outs[k:])


class _CondFactorsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, meta, front, thr, *rows):
        lib = _lib.require_device()
        n_obj, n_con, P, T, coef_c, coef_1mc = meta
        rows = [_prep(r.reshape(-1)) for r in rows]
        if len(rows) != 2 * (n_obj + n_con) or any(r.numel() != T for r in rows):
            raise _lib.MobocmfError("cond_factors: one mean and one variance row of T entries per objective / constraint")
        dev = rows[0].device
        fm, fv = rows[:n_obj], rows[n_obj:2 * n_obj]
        cm, cv = rows[2 * n_obj:2 * n_obj + n_con], rows[2 * n_obj + n_con:]
        grads = _empty(len(rows), T, device=dev)
        g = [grads[i] for i in range(len(rows))]
        loss = _empty((), device=dev)
        front = None if front is None else _prep(front)
        thr = None if thr is None else _prep(thr)
        rc = lib.mobocmf_cond_factors_forward(n_obj, n_con, P, T, _ptr_table(fm), _ptr_table(fv), _ptr_table(cm), _ptr_table(cv),
                                              _ptr(front), _ptr(thr), coef_c, coef_1mc, _ptr(loss),
                                              _ptr_table(g[:n_obj]), _ptr_table(g[n_obj:2 * n_obj]),
                                              _ptr_table(g[2 * n_obj:2 * n_obj + n_con]), _ptr_table(g[2 * n_obj + n_con:]),
                                              _stream())
        _lib.check(rc, "mobocmf_cond_factors_forward")
        ctx.save_for_backward(grads)
        return loss

    @staticmethod
    def backward(ctx, g):
        lib = _lib.require_device()
        (grads,) = ctx.saved_tensors
        n, T = grads.shape
        out = _empty(n, T, device=grads.device)
        one = (ctypes.c_int64 * 1)(n * T)
        _lib.check(lib.mobocmf_scale_segments(1, _ptr_table([grads]), _ptr_table([out]), one, None, _ptr(_prep(g)), _stream()),
                   "mobocmf_scale_segments")
        return (None, None, None) + tuple(out[i] for i in range(n))


def cond_factors(fs_mean, fs_var, cs_mean, cs_var, front, thr, coef_c, coef_1mc):
    """sum_{p, t} [coef_c c + coef_1mc (1 - c)], c(p, t) = prod_k Phi((cs_mean_k[t] - thr_k) / sd) prod_j Phi((front[p, j] -
    fs_mean_j[t]) / sd): the omega factors (blackbox_mfdgp_fitter.py:235-243; coef_c = log eps) and, with no objective rows and
    P = 1, the theta factors (:227-233; coef_c = log(1 - eps)).  Lists of row tensors (T entries each); one launch forward
    (which also forms the gradients), one backward."""
    n_obj, n_con = len(fs_mean), len(cs_mean)
    T = (fs_mean[0] if n_obj else cs_mean[0]).numel()
    P = front.shape[0] if (front is not None and n_obj) else 1
    meta = (n_obj, n_con, int(P), int(T), float(coef_c), float(coef_1mc))
    return _CondFactorsFn.apply(meta, front if n_obj else None, thr if n_con else None,
                                *(list(fs_mean) + list(fs_var) + list(cs_mean) + list(cs_var)))


class _ScalarCombineFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, coefs, *terms):
        lib = _lib.require_device()
        terms = [_prep(t.reshape(1)) for t in terms]
        n = len(terms)
        out = _empty((), device=terms[0].device)
        ctx.coefs, ctx.dev = tuple(float(c) for c in coefs), terms[0].device
        _lib.check(lib.mobocmf_scalar_combine(n, _ptr_table(terms), (ctypes.c_double * n)(*ctx.coefs), _ptr(out), _stream()),
                   "mobocmf_scalar_combine")
        return out

    @staticmethod
    def backward(ctx, g):
        lib = _lib.require_device()
        n = len(ctx.coefs)
        one = _ones_scalar(ctx.dev)
        out = _empty(n, device=ctx.dev)
        sizes = (ctypes.c_int64 * n)(*([1] * n))
        _lib.check(lib.mobocmf_scale_segments(n, _ptr_table([one] * n), _ptr_table([out[i:i + 1] for i in range(n)]), sizes,
                                              (ctypes.c_double * n)(*ctx.coefs), _ptr(_prep(g)), _stream()),
                   "mobocmf_scale_segments")
        return (None,) + tuple(out[i] for i in range(n))


_ones = {}


def _ones_scalar(dev):
    t = _ones.get(dev)
    if t is None:
        t = torch.ones(1, dtype=torch.float64, device=dev)
        _ones[dev] = t
    return t


SEG_MAX = 32      # segments one mobocmf_scalar_combine / _scale_segments / _gather_segments launch takes


def scalar_combine(terms, coefs):
    """sum_i coefs[i] * terms[i] for 0-dim device tensors: one launch (and one for all the terms' gradients); more than
    SEG_MAX terms (a conditioned loss over 16+ black-boxes on one rank) are combined in chunks, then the chunk sums."""
    terms, coefs = list(terms), list(coefs)
    while len(terms) > SEG_MAX:
        part = [_ScalarCombineFn.apply(tuple(coefs[i:i + SEG_MAX]), *terms[i:i + SEG_MAX]) for i in range(0, len(terms), SEG_MAX)]
        terms, coefs = part, [1.0] * len(part)
    return _ScalarCombineFn.apply(tuple(coefs), *terms)


class _AcqMomentsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mu_t, var_t, S):
        lib = _lib.require_device()
        mu_t, var_t = _prep(mu_t.reshape(-1)), _prep(var_t.reshape(-1))
        T = mu_t.numel() // S
        mus = _empty(T, device=mu_t.device)
        vs = _empty_like(mus)
        _lib.check(lib.mobocmf_acq_moments_forward(_ptr(mu_t), _ptr(var_t), _ptr(mus), _ptr(vs), T, S, _stream()),
                   "mobocmf_acq_moments_forward")
        ctx.save_for_backward(mu_t)
        ctx.S = S
        return mus, vs

    @staticmethod
    def backward(ctx, g_mus, g_vars):
        lib = _lib.require_device()
        (mu_t,) = ctx.saved_tensors
        g_mus, g_vars = _prep(g_mus), _prep(g_vars)
        gm, gv = _empty_like(mu_t), _empty_like(mu_t)
        _lib.check(lib.mobocmf_acq_moments_backward(_ptr(mu_t), _ptr(g_mus), _ptr(g_vars), _ptr(gm), _ptr(gv),
                                                    mu_t.numel() // ctx.S, ctx.S, _stream()),
                   "mobocmf_acq_moments_backward")
        return gm, gv, None


def acq_moments(mu_t, var_t, S):
    """mus, vars over the S samples of each test point (mfdgp.py:258-260)."""
    return _AcqMomentsFn.apply(mu_t, var_t, S)


class _JesFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vu, vc):
        lib = _lib.require_device()
        vu, vc = _prep(vu.reshape(-1)), _prep(vc.reshape(-1))
        out = _empty_like(vu)
        _lib.check(lib.mobocmf_jes_forward(_ptr(vu), _ptr(vc), _ptr(out), vu.numel(), _stream()), "mobocmf_jes_forward")
        ctx.save_for_backward(vu, vc, out)
        return out

    @staticmethod
    def backward(ctx, g):
        vu, vc, out = ctx.saved_tensors
        act = (out > 0).to(g.dtype) * g * 0.5
        return act / vu, -act / vc


def jes(v_uncond, v_cond):
    """0.5 * clamp(log v_uncond - log v_cond, min=0)   (JESMOC_MFDGP.py:52)."""
    return _JesFn.apply(v_uncond, v_cond)


def adam_step(param, grad, exp_avg, exp_avg_sq, step, lr, beta1=0.9, beta2=0.999, eps=1e-8, mask=None):
    """In-place fused Adam on flat float64 buffers (torch.optim.Adam semantics)."""
    lib = _lib.require_device()
    _lib.check(lib.mobocmf_adam_step(_ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), _ptr(mask),
                                     param.numel(), lr, beta1, beta2, eps, int(step), _stream()), "mobocmf_adam_step")


class FusedAdam:
    """torch.optim.Adam (defaults: no weight decay, no amsgrad) over all parameters of a model in ONE launch of
    mobocmf_adam_multi, with the step count on the device: capturable, and the update a captured graph replays.
    Duck-types the little of torch.optim.Optimizer the fitter uses (zero_grad / step / state)."""

    def __init__(self, params, lr, betas=(0.9, 0.999), eps=1e-8):
        self.params = [p for group in params for p in group["params"]] if params and isinstance(params[0], dict) \
            else list(params)
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        dev = self.params[0].device
        self.steps_done = torch.zeros((), dtype=torch.int64, device=dev)
        self.state = {"__step__": {"step": self.steps_done}}
        for i, p in enumerate(self.params):
            if p.dtype != torch.float64 or not p.is_cuda:
                raise _lib.MobocmfError("FusedAdam: float64 GPU parameters only")
            self.state[i] = {"exp_avg": torch.zeros_like(p, memory_format=torch.contiguous_format),
                             "exp_avg_sq": torch.zeros_like(p, memory_format=torch.contiguous_format)}

    def zero_grad(self, set_to_none=True):
        for p in self.params:
            if set_to_none:
                p.grad = None
            elif p.grad is not None:
                p.grad.zero_()

    def step(self, exclude=()):
        """``exclude``: ids of parameters another update takes this step (FusedNatGradAdam)."""
        lib = _lib.require_device()
        idx = [i for i, p in enumerate(self.params) if p.grad is not None and id(p) not in exclude]
        if not idx:
            return
        n = len(idx)
        arr = lambda vals: (ctypes.c_void_p * n)(*vals)
        grads = [self.params[i].grad if self.params[i].grad.is_contiguous() else self.params[i].grad.contiguous() for i in idx]
        for i in idx:
            if not self.params[i].is_contiguous():
                raise _lib.MobocmfError("FusedAdam: parameters must be contiguous")
        P = arr([self.params[i].data_ptr() for i in idx])
        G = arr([g.data_ptr() for g in grads])
        M = arr([self.state[i]["exp_avg"].data_ptr() for i in idx])
        V = arr([self.state[i]["exp_avg_sq"].data_ptr() for i in idx])
        N = (ctypes.c_int64 * n)(*[self.params[i].numel() for i in idx])
        _lib.check(lib.mobocmf_adam_multi(n, P, G, M, V, N, self.lr, self.betas[0], self.betas[1], self.eps,
                                          _ptr(self.steps_done), _stream()), "mobocmf_adam_multi")


def natgrad_step(ms, LSs, g_ms, g_LSs, gamma, gamma_init, warmup_steps, scale, step_count, skipped, info):
    """mobocmf_natgrad_step: the natural-gradient update of q(u) = N(m, L_S L_S^T) for the layers of the lists (equal M, at most
    ``_lib.NATGRAD_MAX_LAYERS``), in place.  ``g_ms`` / ``g_LSs``: the loss gradients; ``scale`` turns the loss into -ELBO
    (num_data / batch rows for VariationalELBOMF's loss: 1 on the full batch).  ``step_count``: one device int64 (drives the gamma schedule, incremented); ``skipped`` /
    ``info``: int32 tensors with one word per layer, or lists of one-element int32 tensors (``skipped`` counts the steps a layer was left unchanged because
    I + 2 gamma Psi was not positive definite, ``info`` is that factorisation's pivot report).  Only enqueues: capturable."""
    lib = _lib.require_device()
    n = len(ms)
    if not (len(LSs) == len(g_ms) == len(g_LSs) == n) or n < 1:
        raise _lib.MobocmfError("natgrad_step: one m, L_S, g_m and g_LS per layer")
    M = ms[0].numel()
    for m, L, gm, gL in zip(ms, LSs, g_ms, g_LSs):
        for t in (m, L, gm, gL):
            if not t.is_cuda or t.dtype != torch.float64 or not t.is_contiguous():
                raise _lib.MobocmfError("natgrad_step: contiguous float64 GPU tensors only (there is no CPU fallback)")
        if m.numel() != M or tuple(L.shape) != (M, M) or gm.numel() != M or tuple(gL.shape) != (M, M):
            raise _lib.MobocmfError("natgrad_step: the layers of one call share M (m [M], L_S [M x M])")
    if step_count.dtype != torch.int64 or step_count.numel() != 1 or not step_count.is_cuda:
        raise _lib.MobocmfError("natgrad_step: step_count is one int64 on the GPU")
    words = lambda w: [w.reshape(-1)[z:z + 1] for z in range(w.numel())] if torch.is_tensor(w) else list(w)
    skipped, info = words(skipped), words(info)
    for w in skipped + info:
        if w.dtype != torch.int32 or w.numel() != 1 or not w.is_cuda:
            raise _lib.MobocmfError("natgrad_step: skipped and info hold one int32 per layer on the GPU")
    if len(skipped) != n or len(info) != n:
        raise _lib.MobocmfError("natgrad_step: skipped and info hold one int32 per layer on the GPU")
    nbytes = ctypes.c_size_t()
    _lib.check(lib.mobocmf_natgrad_workspace_bytes(M, n, ctypes.byref(nbytes)), "mobocmf_natgrad_workspace_bytes")
    ws = scratch_buffer(nbytes.value, ms[0].device)
    arr = lambda vals: (ctypes.c_void_p * n)(*vals)
    tn = current_tuning()
    _lib.check(lib.mobocmf_natgrad_step(n, M, arr([t.data_ptr() for t in ms]), arr([t.data_ptr() for t in LSs]),
                                        arr([t.data_ptr() for t in g_ms]), arr([t.data_ptr() for t in g_LSs]), float(gamma),
                                        float(gamma_init), int(warmup_steps), float(scale), _ptr(step_count),
                                        arr([w.data_ptr() for w in skipped]), arr([w.data_ptr() for w in info]),
                                        _ptr(ws), nbytes.value,
                                        ctypes.byref(tn), _stream()), "mobocmf_natgrad_step")


class FusedNatGradAdam:
    """Natural gradients for q(u), Adam for the rest.  Every layer of ``model_or_models`` (one model -- anything with
    ``_layers()`` / ``parameters()`` -- or a list / tuple of them) whose ``variational_mean`` AND ``chol_variational_covar`` both carry a
    gradient in a step is moved by ``natgrad_step``; every other parameter -- and the mean of a layer whose L_S is frozen --
    by the one ``mobocmf_adam_multi`` launch of FusedAdam.  ``elbo_scale`` (a number, or one per model) is the factor between
    the loss the gradients are of and (an unbiased estimate of) -ELBO: VariationalELBOMF returns the data terms summed over the
    batch minus (batch / num_data) KL, so the factor is num_data / batch -- 1 on the full batch and for the conditioned loss;
    ``set_elbo_scale`` changes it between steps (the mini-batch step's ragged batch).  With it gamma = 1 is the exact conjugate
    step.  Layers are grouped by (M, elbo_scale) in calls of at most ``_lib.NATGRAD_MAX_LAYERS``; each call has its own device
    step counter for the gamma schedule.  The counters live in ``state`` with Adam's moments, so what snapshots, rolls
    back or zeroes the optimiser state covers them.  Duck-types FusedAdam (zero_grad / step / state)."""

    def __init__(self, model_or_models, lr, betas=(0.9, 0.999), eps=1e-8, gamma=0.1, gamma_init=1e-4, warmup_steps=100,
                 elbo_scale=1.0):
        models = list(model_or_models) if isinstance(model_or_models, (list, tuple)) else [model_or_models]
        scales = list(elbo_scale) if isinstance(elbo_scale, (list, tuple)) else [elbo_scale] * len(models)
        if len(scales) != len(models) or not all(float(sc) > 0.0 for sc in scales):
            raise ValueError("FusedNatGradAdam: one positive elbo_scale per model")
        self.gamma, self.gamma_init, self.warmup_steps = float(gamma), float(gamma_init), int(warmup_steps)
        if not (self.gamma > 0.0 and 0.0 < self.gamma_init <= self.gamma and self.warmup_steps >= 0):
            raise ValueError("FusedNatGradAdam: 0 < gamma_init <= gamma and warmup_steps >= 0")
        params, seen = [], set()
        for mdl in models:
            for p in mdl.parameters():
                if id(p) not in seen:
                    seen.add(id(p))
                    params.append(p)
        if not params or not params[0].is_cuda:
            raise ValueError("FusedNatGradAdam: the natural-gradient update runs on the GPU only (CPU tensors given)")
        self.adam = FusedAdam(params, lr=lr, betas=betas, eps=eps)
        self.params, self.lr, self.betas, self.eps = self.adam.params, self.adam.lr, self.adam.betas, self.adam.eps
        self.steps_done = self.adam.steps_done
        by_key, n_layers = {}, 0
        for mdl, sc in zip(models, scales):
            for layer in mdl._layers():      # layer k of the models, in their order, owns word k of skipped / info
                vd = layer.variational_strategy._variational_distribution
                m, L = vd.variational_mean, vd.chol_variational_covar
                if m.numel() > _lib.NATGRAD_MAX_M:
                    raise ValueError("FusedNatGradAdam: at most %d inducing points per layer" % _lib.NATGRAD_MAX_M)
                by_key.setdefault((m.numel(), float(sc)), []).append((m, L, n_layers))
                n_layers += 1
        self.groups = []      # [M, scale, [(m, L_S, word)]]
        for (M, sc), pairs in by_key.items():
            for k in range(0, len(pairs), _lib.NATGRAD_MAX_LAYERS):
                self.groups.append([M, sc, pairs[k:k + _lib.NATGRAD_MAX_LAYERS]])
        self.num_layers = n_layers
        dev = params[0].device
        self.natgrad_steps = torch.zeros(max(1, len(self.groups)), dtype=torch.int64, device=dev)
        self.words = torch.zeros(2, max(1, n_layers), dtype=torch.int32, device=dev)      # one host copy reads both rows
        self.skipped, self.info = self.words[0], self.words[1]
        self.state = dict(self.adam.state)
        self.state["__natgrad__"] = {"step": self.natgrad_steps, "words": self.words}

    def zero_grad(self, set_to_none=True):
        self.adam.zero_grad(set_to_none)

    def set_elbo_scale(self, value):
        """One factor for every layer from the next ``step`` on (a host value: a captured step bakes it in)."""
        if not float(value) > 0.0:
            raise ValueError("FusedNatGradAdam: elbo_scale must be positive")
        for group in self.groups:
            group[1] = float(value)

    def step(self):
        taken = set()
        calls = []
        for gi, (M, sc, pairs) in enumerate(self.groups):
            live = [(m, L, w) for m, L, w in pairs if m.grad is not None and L.grad is not None]
            if not live:
                continue
            calls.append((gi, sc, live))
            for m, L, _ in live:
                taken.add(id(m))
                taken.add(id(L))
        cont = lambda g: g if g.is_contiguous() else g.contiguous()
        for gi, sc, live in calls:
            natgrad_step([m.data for m, _, _ in live], [L.data for _, L, _ in live], [cont(m.grad) for m, _, _ in live],
                         [cont(L.grad) for _, L, _ in live], self.gamma, self.gamma_init, self.warmup_steps, sc,
                         self.natgrad_steps[gi], [self.skipped[w:w + 1] for _, _, w in live],
                         [self.info[w:w + 1] for _, _, w in live])
        self.adam.step(exclude=taken)

    def skipped_steps(self):
        """Synchronising (one device-to-host copy): per layer, in the order of the models' layers, how many steps left it unchanged
        because I + 2 gamma Psi was not positive definite.  Raises InLaunchWaitAbandoned if the last factorisation of a layer
        abandoned an in-launch wait."""
        skipped, info = self.words.cpu().tolist()
        for piv in info[:self.num_layers]:
            raise_if_abandoned(piv, "natural-gradient step")
        return skipped[:self.num_layers]


class NatGradSmallLayers:
    """The record array of ``natgrad_small_step`` (mobocmf_natgrad_small_layer), built and uploaded once.  ``layers``: one dict
    per layer with the float64 GPU tensors ``m`` [M], ``L_S`` [M x M], ``g_m`` [M], ``g_LS`` [M x M] (contiguous; views into a
    flat gradient are fine), ``scale`` (default 1), and optionally ``step_count`` (one int64), ``skipped``, ``info`` (one int32
    each) -- where a layer gives none of the three, words of the table's own ``natgrad_steps`` / ``skipped`` / ``info``
    tensors, which exist only then (None when every layer brings its words) -- and the guard:
    ``guard_info`` (int32 tensor, every word of it), ``guard_status`` (the producing launch's status word, int32 or int64),
    ``guard_loss`` (one float64).  The table owns the layers' ``work`` buffers and keeps every tensor alive."""

    def __init__(self, layers):
        lib = _lib.require_device()
        n = len(layers)
        if n < 1:
            raise _lib.MobocmfError("natgrad_small_step: at least one layer")
        dev = layers[0]["m"].device
        self.device = dev
        self.natgrad_steps = self.words = self.skipped = self.info = None
        if not all("step_count" in ly and "skipped" in ly and "info" in ly for ly in layers):
            self.natgrad_steps = torch.zeros(n, dtype=torch.int64, device=dev)
            self.words = torch.zeros(2, n, dtype=torch.int32, device=dev)      # one host copy reads both rows
            self.skipped, self.info = self.words[0], self.words[1]
        self.host = (_lib.NatgradSmallLayer * n)()
        self._keep = []
        for z, ly in enumerate(layers):
            m, L, gm, gL = ly["m"], ly["L_S"], ly["g_m"], ly["g_LS"]
            M = m.numel()
            for t in (m, L, gm, gL):
                if not t.is_cuda or t.dtype != torch.float64 or not t.is_contiguous():
                    raise _lib.MobocmfError("natgrad_small_step: contiguous float64 GPU tensors only (there is no CPU fallback)")
            if not (1 <= M <= _lib.NATGRAD_SMALL_MAX_M):
                raise _lib.MobocmfError("natgrad_small_step: 1 <= M <= %d (got %d)" % (_lib.NATGRAD_SMALL_MAX_M, M))
            if L.numel() != M * M or gm.numel() != M or gL.numel() != M * M:
                raise _lib.MobocmfError("natgrad_small_step: m [M], L_S [M x M], g_m [M], g_LS [M x M] per layer")
            step = ly["step_count"] if "step_count" in ly else self.natgrad_steps[z:z + 1]
            skipped = ly["skipped"] if "skipped" in ly else self.skipped[z:z + 1]
            info = ly["info"] if "info" in ly else self.info[z:z + 1]
            if step.dtype != torch.int64 or step.numel() != 1 or not step.is_cuda:
                raise _lib.MobocmfError("natgrad_small_step: step_count is one int64 on the GPU per layer")
            for w in (skipped, info):
                if w.dtype != torch.int32 or w.numel() != 1 or not w.is_cuda:
                    raise _lib.MobocmfError("natgrad_small_step: skipped and info are one int32 on the GPU per layer")
            R = self.host[z]
            R.M, R.scale = M, float(ly.get("scale", 1.0))
            R.m, R.L_S, R.g_m, R.g_LS = m.data_ptr(), L.data_ptr(), gm.data_ptr(), gL.data_ptr()
            R.step_count, R.skipped, R.info = step.data_ptr(), skipped.data_ptr(), info.data_ptr()
            gi, gst, gl = ly.get("guard_info"), ly.get("guard_status"), ly.get("guard_loss")
            if gi is not None:
                if gi.dtype != torch.int32 or not gi.is_cuda or not gi.is_contiguous():
                    raise _lib.MobocmfError("natgrad_small_step: guard_info is a contiguous int32 GPU tensor")
                R.guard_info, R.n_guard_info = gi.data_ptr(), gi.numel()
            if gst is not None:
                if gst.dtype not in (torch.int32, torch.int64) or gst.numel() != 1 or not gst.is_cuda:
                    raise _lib.MobocmfError("natgrad_small_step: guard_status is one int32 / int64 word on the GPU")
                R.guard_status = gst.data_ptr()
            if gl is not None:
                if gl.dtype != torch.float64 or gl.numel() != 1 or not gl.is_cuda:
                    raise _lib.MobocmfError("natgrad_small_step: guard_loss is one float64 on the GPU")
                R.guard_loss = gl.data_ptr()
            wb = ctypes.c_size_t()
            _lib.check(lib.mobocmf_natgrad_small_work_bytes(M, ctypes.byref(wb)), "mobocmf_natgrad_small_work_bytes")
            work = None
            if wb.value:
                work = torch.zeros(wb.value // 8, dtype=torch.float64, device=dev)
                R.work = work.data_ptr()
            self._keep += [m, L, gm, gL, step, skipped, info, gi, gst, gl, work]
        self.n = n
        self._dev_table = torch.frombuffer(bytearray(bytes(self.host)), dtype=torch.uint8).to(dev)


def natgrad_small_step(layers, gamma, gamma_init, warmup_steps, stream=None):
    """mobocmf_natgrad_small_step: the natural-gradient update of every layer of ``layers`` (a ``NatGradSmallLayers``, or the list
    of dicts it is built from) in ONE launch, one workgroup per layer, M <= 128 and free to differ between the layers; each layer
    has its own gamma-schedule counter.  Only enqueues (on ``stream``, default the current one): capturable.  Returns the table."""
    lib = _lib.require_device()
    table = layers if isinstance(layers, NatGradSmallLayers) else NatGradSmallLayers(layers)
    st = _stream() if stream is None else ctypes.c_void_p(stream.cuda_stream)
    _lib.check(lib.mobocmf_natgrad_small_step(ctypes.cast(table.host, ctypes.c_void_p), ctypes.c_void_p(table._dev_table.data_ptr()),
                                              table.n, float(gamma), float(gamma_init), int(warmup_steps), st),
               "mobocmf_natgrad_small_step")
    return table


def _on(stream):
    return _stream() if stream is None else ctypes.c_void_p(stream.cuda_stream)


def _jes_call(name, moments, noise, dims, acq, tail, seeds, x, best_v, best_x, stream):
    """The one call of a JES entry point ``name``: moments, noise, ``dims`` (the box count, K where the entry point has one, T,
    S), ``tail`` (what stands between S and want_seeds: acq, and box_of_point / acq_ld where the entry point has them), then
    the seeds, the tracking and the stream as every one of them takes them."""
    lib = _lib.require_device()
    track = best_v is not None
    _lib.check(getattr(lib, name)(_ptr(moments), _ptr(noise), *dims, *tail, int(seeds is not None), _ptr(seeds), int(track),
                                  _ptr(x), x.shape[-1] if track else 0, _ptr(best_v), _ptr(best_x), _on(stream)), name)
    return acq


def _jes_boxes(who, moments, K):
    """n_boxes of ``moments`` (n_boxes (1 + K), ...); K < 1 is the library's to refuse."""
    if K >= 1 and moments.shape[0] % (1 + K):
        raise _lib.MobocmfError("%s: 1 + K models per black-box (got K = %d, %d models)" % (who, K, moments.shape[0]))
    return moments.shape[0] // max(1 + K, 1)


def jes_group_forward(moments, noise, T, S, acq, seeds=None, x=None, best_v=None, best_x=None, stream=None):
    """mobocmf_jes_group_forward: ``acq`` (T,) = the JES value of every test point from a predict group's raw ``moments``
    (2 n_pairs, 2, T S) and ``noise`` (2 n_pairs,); ``seeds`` given: d acq.sum() / d moments written there; ``best_v`` (T,) /
    ``best_x`` (T, d) given: updated from the iterate ``x`` (T, d) where acq[t] > best_v[t].  One launch, everything in place,
    only enqueues (on ``stream``, default the current one): capturable."""
    return _jes_call("mobocmf_jes_group_forward", moments, noise, (moments.shape[0] // 2, int(T), int(S)), acq, (_ptr(acq),),
                     seeds, x, best_v, best_x, stream)


def jes_mc_group_forward(moments, noise, K, T, S, acq, seeds=None, x=None, best_v=None, best_x=None, stream=None):
    """mobocmf_jes_mc_group_forward: JES averaged over ``K`` sampled Pareto sets.  ``moments`` (n_boxes (1 + K), 2, T S) and
    ``noise`` (n_boxes (1 + K),): per black-box its unconditioned surrogate, then the K conditioned ones; ``acq`` (T,) =
    sum_p (1/K) sum_k 0.5 max(log v_u,p - log v_c,pk, 0).  ``seeds``, ``x``, ``best_v``, ``best_x`` as in ``jes_group_forward``;
    with K = 1 the same bits as that.  One launch, only enqueues (on ``stream``, default the current one): capturable."""
    K = int(K)
    n_boxes = _jes_boxes("jes_mc_group_forward", moments, K)
    return _jes_call("mobocmf_jes_mc_group_forward", moments, noise, (n_boxes, K, int(T), int(S)), acq, (_ptr(acq),), seeds, x,
                     best_v, best_x, stream)


def jes_mc_box_forward(moments, noise, K, T, S, acq, box_of_point=None, seeds=None, x=None, best_v=None, best_x=None, stream=None):
    """mobocmf_jes_mc_box_forward: JES per black-box, term_p = (1/K) sum_k 0.5 max(log v_u,p - log v_c,pk, 0), from ``moments``
    (n_boxes (1 + K), 2, T S) and ``noise`` laid out as for ``jes_mc_group_forward``.  ``box_of_point`` None: ``acq``
    (n_boxes, >= T) with unit column stride -- a column slice of a wider array will do -- gets term_p[t] in row p; no seeds, no
    tracking.  ``box_of_point`` (T,) int32 on the device: ``acq`` (T,) = term_b[t] with b = box_of_point[t]; ``seeds`` given: the
    coupled launch's seeds for the models of box b, 0.0 for every other model; ``best_v`` / ``best_x`` / ``x`` as in
    ``jes_group_forward``.  One launch, only enqueues (on ``stream``, default the current one): capturable."""
    K, T = int(K), int(T)
    n_boxes = _jes_boxes("jes_mc_box_forward", moments, K)
    ld = 0
    if box_of_point is None:
        if acq.dim() == 1:
            acq = acq[None]
        if acq.dim() != 2 or acq.shape[0] != n_boxes or acq.shape[1] < T or (acq.shape[1] > 1 and acq.stride(1) != 1):
            raise _lib.MobocmfError("jes_mc_box_forward: acq (n_boxes, >= T) with unit column stride")
        ld = acq.stride(0) if n_boxes > 1 else max(acq.stride(0), T)      # (the library refuses a row distance below T)
    else:
        if box_of_point.dtype != torch.int32 or box_of_point.numel() != T or not box_of_point.is_contiguous():
            raise _lib.MobocmfError("jes_mc_box_forward: box_of_point (T,) int32, contiguous")
        if acq.numel() < T:
            raise _lib.MobocmfError("jes_mc_box_forward: acq (T,)")
    return _jes_call("mobocmf_jes_mc_box_forward", moments, noise, (n_boxes, K, T, int(S)), acq,
                     (_ptr(box_of_point), _ptr(acq), int(ld)), seeds, x, best_v, best_x, stream)


def ascent_adam_step(x, gx, lo, hi, exp_avg, exp_avg_sq, steps_done, lr, betas=(0.9, 0.999), eps=1e-8, stream=None):
    """mobocmf_ascent_adam_step: one projected Adam ascent step on the iterate ``x`` (T, d), in place, along
    -gx.sum(0) of the group's input gradients ``gx`` (n_models, T, d) -- FusedAdam's update, then the clamp to [lo, hi] (d,);
    ``steps_done``: one device int64, advanced by the launch.  One launch, only enqueues: capturable."""
    lib = _lib.require_device()
    _lib.check(lib.mobocmf_ascent_adam_step(_ptr(x), _ptr(gx), gx.shape[0], x.shape[0], x.shape[1], _ptr(lo), _ptr(hi),
                                            _ptr(exp_avg), _ptr(exp_avg_sq), float(lr), float(betas[0]), float(betas[1]),
                                            float(eps), _ptr(steps_done), _on(stream)), "mobocmf_ascent_adam_step")
    return x


def select_topk(vals, k, out_vals, out_idx, x=None, out_x=None, stream=None):
    """mobocmf_select_topk: the ``k`` largest of ``vals`` (n,) into ``out_vals`` (k,) / ``out_idx`` (k,, int64) in descending
    order, ties to the lower index, NaN last; with ``x`` (n, d) the selected rows into ``out_x`` (k, d).  One launch, only
    enqueues: capturable."""
    lib = _lib.require_device()
    if out_idx.dtype != torch.int64:
        raise _lib.MobocmfError("select_topk: out_idx must be int64")
    _lib.check(lib.mobocmf_select_topk(_ptr(vals), vals.numel(), int(k), _ptr(x), 0 if x is None else x.shape[-1],
                                       _ptr(out_vals), _ptr(out_idx), _ptr(out_x), _on(stream)), "mobocmf_select_topk")
    return out_vals, out_idx


def mes_group_forward(moments, noise, best, n_obj, n_con, T, acq, seeds=None, x=None, best_v=None, best_x=None, stream=None):
    """mobocmf_mes_group_forward: ``acq`` (T,) = the MES value of every test point from the latent ``moments``
    (n_obj + n_con, 2, T) of exact-GP surrogates, objectives first, their likelihood ``noise`` and ``best`` (best value per
    objective, threshold per constraint): (sum of the objectives' terms) x (product of the constraints' probabilities of
    feasibility), the expressions of MESMOC_MFGP's ``_MES_MFGP.forward``.  ``seeds``, ``x``, ``best_v``, ``best_x`` as in
    ``jes_group_forward``.  One launch, only enqueues (on ``stream``, default the current one): capturable."""
    return _jes_call("mobocmf_mes_group_forward", moments, noise, (_ptr(best), int(n_obj), int(n_con), int(T)), acq, (_ptr(acq),),
                     seeds, x, best_v, best_x, stream)


def exact_predict_work_bytes(model, mode):
    """mobocmf_exact_predict_work_bytes of one ``_lib.ExactPredictModel`` record: the bytes of its ``work`` for ``mode``."""
    nb = ctypes.c_size_t()
    _lib.check(_lib.load().mobocmf_exact_predict_work_bytes(ctypes.byref(model), int(mode), ctypes.byref(nb)),
               "mobocmf_exact_predict_work_bytes")
    return nb.value


def exact_predict_launch(host_models, dev_table, mode, stream=None):
    """mobocmf_exact_predict: ``host_models`` a ctypes array of ``_lib.ExactPredictModel``, ``dev_table`` the same bytes in a
    device uint8 tensor; ``mode`` _lib.STEP_FORWARD or _lib.STEP_INPUT_GRADIENTS.  One launch, only enqueues (on ``stream``,
    default the current one): capturable after the first call of each mode."""
    lib = _lib.require_device()
    _lib.check(lib.mobocmf_exact_predict(ctypes.cast(host_models, ctypes.c_void_p), _ptr(dev_table), len(host_models), int(mode),
                                         _on(stream)), "mobocmf_exact_predict")


def exact_fit_work_bytes(model, n_models=1):
    """mobocmf_exact_fit_work_bytes of one ``_lib.ExactFitModel`` record (of a table of ``n_models``): the bytes of its ``work``."""
    nb = ctypes.c_size_t()
    _lib.check(_lib.load().mobocmf_exact_fit_work_bytes(ctypes.byref(model), int(n_models), ctypes.byref(nb)),
               "mobocmf_exact_fit_work_bytes")
    return nb.value


def _exact_fit_call(name, host_models, dev_table, stream, *args):
    lib = _lib.require_device()
    _lib.check(getattr(lib, name)(ctypes.cast(host_models, ctypes.c_void_p), _ptr(dev_table), len(host_models), *args, _on(stream)),
               name)


def exact_fit_covariance(host_models, dev_table, stream=None):
    """mobocmf_exact_fit_covariance: the padded training covariance of every model of the table from its current raw parameters,
    into the models' work areas.  One launch, only enqueues (``host_models`` a ctypes array of ``_lib.ExactFitModel``,
    ``dev_table`` the same bytes in a device uint8 tensor -- as for ``exact_predict_launch``)."""
    _exact_fit_call("mobocmf_exact_fit_covariance", host_models, dev_table, stream)


def exact_fit_prepare(host_models, dev_table, stream=None):
    """mobocmf_exact_fit_prepare: L^-T and alpha = L^-T a of every model from its factorisation's state.  One launch."""
    _exact_fit_call("mobocmf_exact_fit_prepare", host_models, dev_table, stream)


def exact_fit_gradient(host_models, dev_table, stream=None):
    """mobocmf_exact_fit_gradient: every model's slab of partial sums sum_ij G_ij dK_ij / dvalue.  One launch, no atomics."""
    _exact_fit_call("mobocmf_exact_fit_gradient", host_models, dev_table, stream)


def exact_fit_update(host_models, dev_table, mode, lr, betas=(0.9, 0.999), eps=1e-8, stream=None):
    """mobocmf_exact_fit_update: ``mode`` _lib.EXACT_FIT_STEP (slab sum, stop / best bookkeeping, chain rule, Adam through the
    pointer table) or _lib.EXACT_FIT_FINISH (the restore decision).  One launch."""
    _exact_fit_call("mobocmf_exact_fit_update", host_models, dev_table, stream, int(mode), float(lr), float(betas[0]),
                    float(betas[1]), float(eps))


def exact_sample_gram(host_problems, dev_table, stream=None):
    """mobocmf_exact_sample_gram: G = Phi^T Phi + noise I (padded for the factorisation) and r = y - Phi^T theta0 - e of every
    (model, sample) problem of the table.  One launch, only enqueues (``host_problems`` a ctypes array of
    ``_lib.ExactSampleProblem``, ``dev_table`` the same bytes in a device uint8 tensor)."""
    _exact_fit_call("mobocmf_exact_sample_gram", host_problems, dev_table, stream)


def exact_sample_weights(host_problems, dev_table, stream=None):
    """mobocmf_exact_sample_weights: w = L^-T a, theta = theta0 + Phi w and the packed one-layer chain samples of the requested
    output levels; copies each factorisation's info word next to the others.  Two launches, only enqueues."""
    _exact_fit_call("mobocmf_exact_sample_weights", host_problems, dev_table, stream)


def check_info(info):
    """Synchronising: raises if the last Cholesky reported a non-positive pivot."""
    lib = _lib.require_device()
    piv = ctypes.c_int32()
    rc = lib.mobocmf_check_info(_ptr(info), ctypes.byref(piv), _stream())
    if rc == _lib.NOT_PD:
        return piv.value
    _lib.check(rc, "mobocmf_check_info")
    return 0


class InLaunchWaitAbandoned(FloatingPointError):
    """A one-launch form (cooperative step, one-launch Cholesky) gave up a bounded in-launch wait: its workgroups were not resident
    together (too many such launches in flight on the device, or a partition with few CUs).  The call's results are invalid."""


class InLaunchSync:
    """The device words of a one-launch form whose counters persist across launches (the cooperative step, the conditioned
    iteration): arrival counters and, at ``status_index``, the status word its launches only ever OR (include/mobocmf_hip.h,
    mobocmf_coop_elbo_step).  Only this owner clears them, all together.  ``stream``: the one the launches run on (None: the
    current stream)."""

    def __init__(self, words, status_index, stream=None):
        self.words, self.status_index, self.stream = words, status_index, stream

    def ptr(self, index):
        return self.words[index].data_ptr()

    def _stream(self):
        return self.stream if self.stream is not None else torch.cuda.current_stream(self.words.device)

    def check(self, what):
        """Synchronising: raises InLaunchWaitAbandoned if a launch since the last reset gave up a wait (the words are cleared)."""
        self._stream().synchronize()
        st = int(self.words[self.status_index].item())
        if st:
            self.reset()
            raise InLaunchWaitAbandoned("%s: %s (status %d)" % (what, "a workgroup gave up an in-launch wait" if st & 1 else
                                                                "the launch did not match its coupling record", st))

    def reset(self):
        """Zeroes the counters and the status word, ordered with the launches on the owner's stream."""
        with torch.cuda.stream(self._stream()):
            self.words.zero_()


def raise_if_abandoned(pivot, what="Cholesky"):
    """``pivot`` as returned by check_info: -1 is not a failed pivot but an abandoned in-launch wait (include/mobocmf_hip.h,
    mobocmf_check_info)."""
    if pivot < 0:
        raise InLaunchWaitAbandoned("%s: the one-launch form abandoned a bounded in-launch wait (its workgroups were not resident "
                                    "together); repeat the call with F.tuning(potrf_cols=4) or less concurrent work" % what)


def gemm_colstat_rows(Mr, Nc, Kd, tri=0, tune=None):
    """Partial rows the column-statistics epilogue writes for a product of that shape (two per row block of the tile
    height the tuning gives: mobocmf_gemm_colstat_rows)."""
    rows = ctypes.c_int32()
    snap = tune if tune is not None else current_tuning()
    _lib.check(_lib.load().mobocmf_gemm_colstat_rows(tri, Mr, Nc, Kd, ctypes.byref(snap), ctypes.byref(rows)),
               "mobocmf_gemm_colstat_rows")
    return rows.value


# ---- host-side defaults of the knobs (process-wide in THIS module; the library itself holds nothing -- see `tuning` above).
def set_mid_gemm_max(n=1024):
    """Largest dimension of a plain product that runs on the mid-size (one launch, no k-slicing) kernel; 0 = off."""
    if not 0 <= int(n) <= 4096:
        raise _lib.MobocmfError("set_mid_gemm_max: 0..4096")
    _set_default(mid_gemm_max=n)


def set_mid_gemm_waves(n=32):
    """Form of the mid-size product kernel: 32 (32 x 64 tiles, 64-k stages; default), 8 or 4 (64 x 64 tiles on that many
    wavefronts)."""
    if int(n) not in (4, 8, 32):
        raise _lib.MobocmfError("set_mid_gemm_waves: 4 | 8 | 32")
    _set_default(mid_gemm_waves=n)


def set_syrk_workgroups(n=0):
    """Workgroups a k-sliced weighted syrk may occupy (0 = by shape).  Sizes follow the tuning a call carries."""
    if int(n) != 0 and not 16 <= int(n) <= 4096:
        raise _lib.MobocmfError("set_syrk_workgroups: 0 | 16..4096")
    _set_default(syrk_workgroups=n)


def set_sparse_backward(on=True):
    """Skip the 128-column blocks of a layer backward whose upstream gradients are all exactly zero (default on).  Off = the
    dense backward: A/B timing and the parity tests.  Read when the FORWARD of a layer call is issued."""
    _set_default(sparse_backward=1 if on else 0)


_block_act_tls = threading.local()


def set_block_activity(act=None):
    """Tests / tools: int32 CUDA tensor (one word per 128 columns) that the standalone gemm_f64_epilogue / syrk_weighted calls
    of THIS thread pass as their col_activity / k_activity argument until it is cleared with None."""
    if act is not None:
        assert act.dtype == torch.int32 and act.is_cuda and act.is_contiguous()
    _block_act_tls.act = act


def set_tile_rows(rows=0, pair_mode=0):
    """Tile height of the M x N' panel products: 0 automatic, 64 or 128; row-block pairing 0 automatic, 1 never, 2 always."""
    if int(rows) not in (0, 64, 128) or not 0 <= int(pair_mode) <= 2:
        raise _lib.MobocmfError("set_tile_rows: rows 0 | 64 | 128, pair_mode 0..2")
    _set_default(tile_rows=rows, pair_mode=pair_mode)


def set_potrf_cols(cols=0):
    """The blocked Cholesky: 0 (default) all 64-column steps in one launch where it applies; 4 or 1: a launch pair per 64
    columns with that many columns per hand-over of the panel kernel."""
    if int(cols) not in (0, 1, 4):
        raise _lib.MobocmfError("set_potrf_cols: 0 | 1 | 4")
    _set_default(potrf_cols=cols)


def set_tuning(small_gemm_max=0, small_panel_max=0):
    """Kernel-selection thresholds (size sweeps); 0 leaves a threshold unchanged."""
    if int(small_gemm_max) > 512 or int(small_panel_max) > 512:
        raise _lib.MobocmfError("set_tuning: the small kernels serve dimensions <= 512")
    if small_gemm_max > 0:
        _set_default(small_gemm_max=small_gemm_max)
    if small_panel_max > 0:
        _set_default(small_panel_max=small_panel_max)


def gemm_f64_epilogue(A, B, C, tri, epi, alpha=1.0, stream_out=False, colsq_part=None, coldot_part=None, avec=None,
                      bscale=None, gmu=None, cgv=None, Aaux=None, rowdot_part=None):
    """The GEMM with the epilogue the layer launches it with (mobocmf_gemm_f64_epilogue): tests and per-variant timing."""
    lib = _lib.require_device()
    A, B = _prep(A), _prep(B)
    Mr, Kd = A.shape
    Nc = B.shape[1]
    snap = current_tuning()
    if epi == 1:
        need = gemm_colstat_rows(Mr, Nc, Kd, tri, tune=snap) * Nc
        for part in (colsq_part, coldot_part):
            if part is not None and part.numel() < need:
                raise _lib.MobocmfError("gemm_f64_epilogue: the partial-statistics buffers need gemm_colstat_rows() = %d rows"
                                        % (need // Nc))
    _lib.check(lib.mobocmf_gemm_f64_epilogue(tri, epi, Mr, Nc, Kd, _ptr(A), A.stride(0), _ptr(B), B.stride(0), _ptr(C),
                                             C.stride(0), alpha, int(stream_out), _ptr(colsq_part), _ptr(coldot_part),
                                             _ptr(avec), _ptr(bscale), _ptr(gmu), _ptr(cgv), _ptr(Aaux), _ptr(rowdot_part),
                                             _ptr(getattr(_block_act_tls, "act", None)), ctypes.byref(snap), _stream()),
               "mobocmf_gemm_f64_epilogue")
    return C


def gram(kind, x1, f1, x2, f2, hyp, xdiv=1, knn=False):
    """Dense k([x1, f1], [x2, f2]) of a layer's kernel (n1 x n2), no autograd: the evaluated prior of
    MFDGPHiddenLayer.forward.  ``xdiv`` > 1: ``x2`` holds base rows, each replicated ``xdiv`` times (column j = row
    j // xdiv of x2 with f2[j]; f2 holds x2.shape[0] * xdiv values) -- the launch of a layer's K_mn
    (mobocmf_gram_forward_rep).  ``knn``: also return the prior variances of the columns, (K, knn)."""
    lib = _lib.require_device()
    with torch.no_grad():
        x1, f1, x2, f2, hyp = (_prep(None if t is None else t.detach()) for t in (x1, f1, x2, f2, hyp))
        n1, nb2, d = x1.shape[0], x2.shape[0], x1.shape[1]
        if not 1 <= int(xdiv) <= _lib.MAX_XDIV:
            raise _lib.MobocmfError("gram: xdiv 1..%d" % _lib.MAX_XDIV)
        n2 = nb2 * int(xdiv)
        if x2.shape[1] != d or hyp.numel() != hyp_len(kind, d) or not 1 <= d <= _lib.MAX_D or \
                (kind == 1 and (f1 is None or f2 is None or f1.numel() != n1 or f2.numel() != n2)):
            raise _lib.MobocmfError("gram: shape mismatch")
        K = _empty((n1 + 31) // 32 * 32, n2, device=x1.device)
        if int(xdiv) == 1 and not knn:
            _lib.check(lib.mobocmf_gram_forward(kind, d, _ptr(x1), _ptr(f1), n1, _ptr(x2), _ptr(f2), n2, _ptr(hyp), _ptr(K),
                                                K.stride(0), _stream()), "mobocmf_gram_forward")
            return K[:n1]
        kd = _empty(n2, device=x1.device) if knn else None
        _lib.check(lib.mobocmf_gram_forward_rep(kind, d, _ptr(x1), _ptr(f1), n1, _ptr(x2), _ptr(f2), nb2, int(xdiv), _ptr(hyp),
                                                _ptr(K), K.stride(0), _ptr(kd), _stream()), "mobocmf_gram_forward_rep")
    return (K[:n1], kd) if knn else K[:n1]


def rff_eval(kind, x, fprev, W1, b1, Wf, W2, b2, theta, s0, s1=0.0, s2=0.0):
    """One RFF function sample of a layer at the rows of ``x`` (n, d) on the GPU (mobocmf_rff_eval); ``fprev`` (n,) = the
    previous layer's sample at the same rows (kind 1).  No autograd."""
    lib = _lib.require_device()
    with torch.no_grad():
        x, fprev, W1, b1, Wf, W2, b2, theta = (_prep(None if t is None else t.detach().reshape(t.shape))
                                               for t in (x, fprev, W1, b1, Wf, W2, b2, theta))
        n, d = x.shape
        Fn = W1.shape[0]
        if W1.shape[1] != d or b1.numel() != Fn or theta.numel() != (Fn if kind == 0 else 3 * Fn):
            raise _lib.MobocmfError("rff_eval: shape mismatch")
        if kind == 1 and (fprev.numel() != n or Wf.numel() != Fn or tuple(W2.shape) != (Fn, d) or b2.numel() != Fn):
            raise _lib.MobocmfError("rff_eval: shape mismatch (layer >= 1 operands)")
        out = _empty(n, device=x.device)
        _lib.check(lib.mobocmf_rff_eval(kind, d, Fn, n, _ptr(x), _ptr(fprev), _ptr(W1), _ptr(b1), _ptr(Wf), _ptr(W2),
                                        _ptr(b2), _ptr(theta), float(s0), float(s1), float(s2), _ptr(out), _stream()),
                   "mobocmf_rff_eval")
    return out


def _rff_chain_table(what, layers, d, plen, device):
    """The DEVICE table of mobocmf_rff_layer_desc of ``layers`` (see ``rff_eval_chains``), every shape and offset checked
    against ``plen`` doubles of params here, on the host."""
    Lmax = _lib.RFF_MAX_LAYERS
    K = len(layers)
    tab = (_lib.RffLayerDesc * (K * Lmax))()
    for k, chain in enumerate(layers):
        if not 1 <= len(chain) <= Lmax:
            raise _lib.MobocmfError("%s: a chain sample has 1..%d layers" % (what, Lmax))
        for l in range(Lmax):
            e = tab[k * Lmax + l]
            if l >= len(chain):
                e.kind = -1
                continue
            L = chain[l]
            kind, Fn = int(L["kind"]), int(L["F"])
            if kind != (0 if l == 0 else 1) or Fn < 1:
                raise _lib.MobocmfError("%s: layer 0 is kind 0, the layers above it kind 1" % what)
            need = {"W1": Fn * d, "b1": Fn, "theta": Fn if kind == 0 else 3 * Fn}
            if kind == 1:
                need.update({"Wf": Fn, "W2": Fn * d, "b2": Fn})
            for name, cnt in need.items():
                off = int(L[name])
                if off < 0 or off + cnt > plen:
                    raise _lib.MobocmfError("%s: operand %s of sample %d layer %d lies outside params" % (what, name, k, l))
                setattr(e, name, off)
            e.kind, e.F = kind, Fn
            e.s0, e.s1, e.s2 = float(L["s0"]), float(L.get("s1", 0.0)), float(L.get("s2", 0.0))
    return torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(device)


def _rff_chain_args(what, x, params, layers):
    """(x, params, n, d, K, plen) of a call on chain samples, checked as ``rff_eval_chains`` documents."""
    if not (torch.is_tensor(x) and torch.is_tensor(params)) or x.dim() != 2 or params.dim() != 1 or params.device != x.device \
            or x.device.type != "cuda":
        raise _lib.MobocmfError("%s: x must be (n, d) and params 1-D, on one GPU" % what)
    x, params = _prep(x.detach()), _prep(params.detach())
    n, d = x.shape
    K, plen = len(layers), params.numel()
    if not 1 <= K <= 65535 or n < 1 or not 1 <= d <= _lib.MAX_D or plen < 1:
        raise _lib.MobocmfError("%s: shape mismatch" % what)
    return x, params, n, d, K, plen


def rff_eval_chains(x, params, layers):
    """K chain samples at the rows of ``x`` (n, d) on the GPU in one launch (mobocmf_rff_eval_chains) -> (K, n).  ``params``:
    1-D float64 device tensor holding every sample's operands; ``layers``: per sample, the list of its layers (layer 0 first),
    each a dict with kind, F, the offsets W1 / b1 / theta (and Wf / W2 / b2 for kind 1) into ``params`` and the scales
    s0 / s1 / s2 of ``rff_eval``.  The shapes are checked here, on the host.  No autograd."""
    lib = _lib.require_device()
    with torch.no_grad():
        x, params = _prep(x.detach()), _prep(params.detach())
        if x.dim() != 2 or params.dim() != 1 or params.device != x.device:
            raise _lib.MobocmfError("rff_eval_chains: x must be (n, d) and params 1-D, on one device")
        n, d = x.shape
        K, plen = len(layers), params.numel()
        if not 1 <= K <= 65535 or n < 1 or not 1 <= d <= _lib.MAX_D or plen < 1:
            raise _lib.MobocmfError("rff_eval_chains: shape mismatch")
        desc = _rff_chain_table("rff_eval_chains", layers, d, plen, x.device)
        out = _empty(K, n, device=x.device)
        _lib.check(lib.mobocmf_rff_eval_chains(K, d, n, _ptr(x), _ptr(params), plen, _ptr(desc), _ptr(out), _stream()),
                   "mobocmf_rff_eval_chains")
    return out


def rff_chains_value_grad(x, params, layers):
    """K chain samples and their input gradients at the rows of ``x`` (n, d) on the GPU in one launch
    (mobocmf_rff_chains_value_grad) -> (vals (K, n), grads (K, n, d)).  Operands and checks: ``rff_eval_chains``.  No
    autograd."""
    lib = _lib.require_device()
    with torch.no_grad():
        x, params, n, d, K, plen = _rff_chain_args("rff_chains_value_grad", x, params, layers)
        desc = _rff_chain_table("rff_chains_value_grad", layers, d, plen, x.device)
        vals, grads = _empty(K, n, device=x.device), _empty(K, n, d, device=x.device)
        _lib.check(lib.mobocmf_rff_chains_value_grad(K, d, n, _ptr(x), _ptr(params), plen, _ptr(desc), _ptr(vals),
                                                     _ptr(grads), _stream()), "mobocmf_rff_chains_value_grad")
    return vals, grads


def rff_refine_options(**kw):
    """The settings of ``rff_refine`` (mobocmf_rff_refine_options): the library's defaults with ``kw`` (outer, inner, backtracks,
    restore, recentre, step0, step_shrink, step_grow, rho0, rho_growth, armijo, restore_margin) replaced."""
    opt = _lib.RffRefineOptions()
    _lib.check(_lib.load().mobocmf_rff_refine_options_init(ctypes.byref(opt)), "mobocmf_rff_refine_options_init")
    for name, v in kw.items():
        if name not in _lib.RffRefineOptions.KNOBS:
            raise _lib.MobocmfError("rff_refine_options: no option %r" % name)
        setattr(opt, name, v)
    return opt


def rff_refine(x0, params, layers, obj, cons=None, thr=None, options=None):
    """Constrained multi-start refinement of chain samples in one launch (mobocmf_rff_refine).  ``x0`` (P, R, d): R starts for
    each of P problems; ``params`` / ``layers``: the chain samples, as for ``rff_eval_chains``; problem p minimises chain
    ``obj[p]`` over [0, 1]^d subject to chain ``cons[p][i]`` (x) >= ``thr[p][i]`` (``cons`` / ``thr``: per problem a sequence,
    possibly empty; None = no constraints); ``options``: ``rff_refine_options(...)`` or a dict of its keywords.  Returns a
    dict of device tensors: per start ``xs`` (P, R, d), ``fs`` (P, R), ``slack_min`` (P, R) -- the best feasible point
    evaluated from that start, NaN ``fs`` if there is none -- and per problem ``x_best`` (P, d), ``f_best`` (P,),
    ``start_best`` (P,) int32, ``status`` (P,) int32 (``_lib.REFINE_STATUS``).  No autograd, no host synchronisation."""
    lib = _lib.require_device()
    with torch.no_grad():
        if not torch.is_tensor(x0) or x0.dim() != 3:
            raise _lib.MobocmfError("rff_refine: x0 must be (P, R, d)")
        P, R, d = x0.shape
        if P < 1 or R < 1:
            raise _lib.MobocmfError("rff_refine: x0 must be (P, R, d) with P, R >= 1")
        xf, params, _, d, K, plen = _rff_chain_args("rff_refine", x0.reshape(P * R, d), params, layers)
        obj = [int(o) for o in obj]
        cons = [[] for _ in obj] if cons is None else [[int(c) for c in cs] for cs in cons]
        thr = [[] for _ in obj] if thr is None else [torch.as_tensor(ts, dtype=torch.float64).reshape(-1).tolist()
                                                     for ts in thr]
        if len(obj) != P or len(cons) != P or len(thr) != P or not 1 <= P <= _lib.REFINE_MAX_PROBLEMS:
            raise _lib.MobocmfError("rff_refine: one objective, one constraint list and one threshold list per problem "
                                    "(at most %d problems)" % _lib.REFINE_MAX_PROBLEMS)
        for p in range(P):
            if not 0 <= obj[p] < K or any(not 0 <= c < K for c in cons[p]):
                raise _lib.MobocmfError("rff_refine: problem %d names a chain outside 0..%d" % (p, K - 1))
            if len(cons[p]) != len(thr[p]) or len(cons[p]) > _lib.REFINE_MAX_CON:
                raise _lib.MobocmfError("rff_refine: problem %d needs one threshold per constraint (at most %d)"
                                        % (p, _lib.REFINE_MAX_CON))
        if isinstance(options, dict):
            options = rff_refine_options(**options)
        cnt = [len(c) for c in cons]
        off = [sum(cnt[:p]) for p in range(P)]
        n_con = sum(cnt)
        i32 = lambda v: (ctypes.c_int32 * len(v))(*v)
        dev = xf.device
        con_d = torch.tensor([c for cs in cons for c in cs], dtype=torch.int32).to(dev) if n_con else None
        thr_d = torch.tensor([t for ts in thr for t in ts], dtype=torch.float64).to(dev) if n_con else None
        desc = _rff_chain_table("rff_refine", layers, d, plen, dev)
        out = {"xs": _empty(P, R, d, device=dev), "fs": _empty(P, R, device=dev), "slack_min": _empty(P, R, device=dev),
               "x_best": _empty(P, d, device=dev), "f_best": _empty(P, device=dev),
               "start_best": torch.empty(P, dtype=torch.int32, device=dev),
               "status": torch.empty(P, dtype=torch.int32, device=dev)}
        _lib.check(lib.mobocmf_rff_refine(P, R, d, K, i32(obj), i32(off), i32(cnt), n_con, _ptr(con_d), _ptr(thr_d), _ptr(xf),
                                          _ptr(params), plen, _ptr(desc),
                                          None if options is None else ctypes.byref(options),
                                          *[_ptr(out[k]) for k in ("xs", "fs", "slack_min", "x_best", "f_best", "start_best",
                                                                   "status")], _stream()), "mobocmf_rff_refine")
    return out


def rff_feasibility(vals, thr):
    """Feasibility of the columns of ``vals`` (K_con, n) -- constraint samples on a grid -- under thresholds ``thr`` (K_con,)
    (mobocmf_rff_feasibility, the rule of MOOP.find_feasible_grid): (ok (n,) bool, every slack >= 0; violation (n,) float64,
    sum of min(slack, 0))."""
    lib = _lib.require_device()
    with torch.no_grad():
        if vals.dim() != 2 or vals.shape[0] < 1 or vals.shape[1] < 1 or thr.numel() != vals.shape[0] \
                or thr.device != vals.device:
            raise _lib.MobocmfError("rff_feasibility: shape mismatch")
        vals, thr = _prep(vals.detach()), _prep(thr.detach().reshape(-1))
        K, n = vals.shape
        ok = torch.empty(n, dtype=torch.int32, device=vals.device)
        viol = _empty(n, device=vals.device)
        _lib.check(lib.mobocmf_rff_feasibility(K, n, _ptr(vals), n, _ptr(thr), _ptr(ok), _ptr(viol), _stream()),
                   "mobocmf_rff_feasibility")
    return ok.bool(), viol


def nsga_options(**kw):
    """The settings of ``nsga_vary`` (mobocmf_nsga_options): the library's defaults with ``kw`` (eta_c, p_c, eta_m, p_m)
    replaced."""
    opt = _lib.NsgaOptions()
    _lib.check(_lib.load().mobocmf_nsga_options_init(ctypes.byref(opt)), "mobocmf_nsga_options_init")
    for name, v in kw.items():
        if name not in _lib.NsgaOptions.KNOBS:
            raise _lib.MobocmfError("nsga_options: no option %r" % name)
        setattr(opt, name, float(v))
    return opt


def _nsga_opt(options):
    return nsga_options(**options) if isinstance(options, dict) else options


def nsga_survive(X, F, viol=None, n_keep=None, generation=None):
    """Constraint-domination ranks, crowding distances and the ``n_keep`` best of the rows ``X`` (n_in, d) with objective values
    ``F`` (k, n_in) (minimised) and violations ``viol`` (n_in,) (>= 0, 0 = feasible; None: all feasible), in one launch
    (mobocmf_nsga_survive; ``n_keep`` None = n_in, rank only).  ``generation``: a device int64 word the launch increments, or
    None.  Returns a dict of new device tensors in key order (rank, -crowding, row): ``X``, ``F``, ``viol`` (None without
    ``viol``), ``rank`` (int32), ``crowd``, ``src`` (int32, the input row).  No autograd, no host synchronisation."""
    lib = _lib.require_device()
    with torch.no_grad():
        if not (torch.is_tensor(X) and torch.is_tensor(F)) or X.dim() != 2 or F.dim() != 2 or F.shape[1] != X.shape[0] \
                or F.device != X.device:
            raise _lib.MobocmfError("nsga_survive: X must be (n_in, d) and F (k, n_in), on one GPU")
        X, F = _prep(X.detach()), _prep(F.detach())
        n_in, d = X.shape
        k = F.shape[0]
        n_keep = n_in if n_keep is None else int(n_keep)
        if viol is not None:
            if viol.numel() != n_in or viol.device != X.device:
                raise _lib.MobocmfError("nsga_survive: viol must be (n_in,)")
            viol = _prep(viol.detach().reshape(-1))
        if generation is not None and (generation.dtype != torch.int64 or generation.device != X.device):
            raise _lib.MobocmfError("nsga_survive: generation must be a device int64 word")
        dev, m = X.device, max(n_keep, 0)
        out = {"X": _empty(m, d, device=dev), "F": _empty(k, m, device=dev),
               "viol": None if viol is None else _empty(m, device=dev),
               "rank": torch.empty(m, dtype=torch.int32, device=dev), "crowd": _empty(m, device=dev),
               "src": torch.empty(m, dtype=torch.int32, device=dev)}
        _lib.check(lib.mobocmf_nsga_survive(n_in, n_keep, d, k, _ptr(X), _ptr(F), n_in, _ptr(viol), _ptr(out["X"]),
                                            _ptr(out["F"]), max(m, 1), _ptr(out["viol"]), _ptr(out["rank"]), _ptr(out["crowd"]),
                                            _ptr(out["src"]), _ptr(generation), _stream()), "mobocmf_nsga_survive")
    return out


def nsga_vary(X, rank, crowd, seed, generation, options=None):
    """Np children of the ranked parents ``X`` (Np, d) with ``rank`` (int32) / ``crowd`` (Np,) (what ``nsga_survive`` returns):
    binary tournaments, simulated binary crossover, polynomial mutation, clamped to [0, 1] (mobocmf_nsga_vary).  ``seed``: the
    Philox key; ``generation``: a device int64 word, the Philox call counter (``nsga_survive`` increments it); ``options``:
    ``nsga_options(...)`` or a dict of its keywords.  Returns (children (Np, d), parents (Np,) int32 -- the tournament winners,
    two per pair).  No autograd, no host synchronisation."""
    lib = _lib.require_device()
    with torch.no_grad():
        if not torch.is_tensor(X) or X.dim() != 2 or rank.numel() != X.shape[0] or crowd.numel() != X.shape[0] \
                or rank.dtype != torch.int32 or generation.dtype != torch.int64 \
                or len({X.device, rank.device, crowd.device, generation.device}) != 1:
            raise _lib.MobocmfError("nsga_vary: X (Np, d), rank (Np,) int32, crowd (Np,), generation int64, on one GPU")
        X, crowd = _prep(X.detach()), _prep(crowd.detach().reshape(-1))
        rank = rank.contiguous()
        Np, d = X.shape
        children = _empty(Np, d, device=X.device)
        parents = torch.empty(Np, dtype=torch.int32, device=X.device)
        options = _nsga_opt(options)
        _lib.check(lib.mobocmf_nsga_vary(Np, d, _ptr(X), _ptr(rank), _ptr(crowd), int(seed) & (2 ** 64 - 1), _ptr(generation),
                                         None if options is None else ctypes.byref(options), _ptr(children), _ptr(parents),
                                         _stream()), "mobocmf_nsga_vary")
    return children, parents


def rff_evolve(x0, params, layers, n_obj, thr, generations, seed, options=None):
    """NSGA-II on chain samples with no host in the loop (util/pareto_evolve.py ParetoEvolve): the population ``x0`` (Np, d), Np
    even in 4..512, evolves for ``generations`` generations, each ONE graph replay of vary -> mobocmf_rff_eval_chains on the
    children -> mobocmf_rff_feasibility -> survive on the 2 Np rows.  ``params`` / ``layers``: the chain samples as for
    ``rff_eval_chains``, the first ``n_obj`` are the objectives (minimised), the others constraints, feasible when sample >=
    ``thr`` (one threshold each).  Returns a dict of device tensors: ``X`` (Np, d), ``F`` (n_obj, Np), ``viol`` (Np,) (0 =
    feasible), ``rank`` (int32), ``crowd``, ``generation`` (int64 word), in the survivors' key order.  Nothing is read on the
    host."""
    from .util.pareto_evolve import ParetoEvolve
    eng = ParetoEvolve(params, layers, n_obj, thr, x0.shape[0], x0.shape[1], seed, options=options)
    eng.start(x0)
    eng.run(generations)
    return eng.result()


def recommend_z_min(p_min):
    """Phi^-1(p_min): the ``z_min`` of ``recommend_scores`` for the feasibility probability ``p_min`` (0.0 for a ``p_min``
    outside (0, 1): the library refuses that one itself)."""
    import statistics
    p_min = float(p_min)
    return statistics.NormalDist().inv_cdf(p_min) if 0.0 < p_min < 1.0 else 0.0


def recommend_scores(moments, n_obj, T, S, scale=None, p_min=0.999, z_min=None, F=None, viol=None, stream=None):
    """mobocmf_recommend_scores: a predict group's raw ``moments`` (n_obj + n_con, 2, T S) -- objectives first -- as the operands of
    ``nsga_survive``: ``F`` (n_obj, T) the predictive means over the S samples (minimised), ``viol`` (T,) the graded violation of
    ``pareto_mask``'s rule on noise-free variances, 0 exactly where every constraint has Phi(mbar / sqrt(v)) > ``p_min``, else
    sum_c max(z_min - z_c, DBL_MIN) over the failing constraints (+inf for v < 0 or a NaN).  ``scale`` (n_obj + n_con, 2): (shift,
    factor) per model; ``z_min`` None: Phi^-1(p_min).  ``F`` / ``viol`` given: written in place (``F`` may be a column slice of a
    wider array: unit column stride), else new tensors (``viol`` None without constraints).  One launch, only enqueues (on
    ``stream``, default the current one): capturable.  Returns (F, viol)."""
    lib = _lib.require_device()
    with torch.no_grad():
        if not torch.is_tensor(moments) or moments.dim() != 3 or moments.shape[1] != 2 or not moments.is_contiguous() \
                or moments.dtype != torch.float64 or not moments.is_cuda:
            raise _lib.MobocmfError("recommend_scores: moments must be a contiguous (n_obj + n_con, 2, T S) float64 tensor on a GPU")
        n_obj, T, S = int(n_obj), int(T), int(S)
        n_con = moments.shape[0] - n_obj
        if T >= 1 and S >= 1 and moments.shape[2] != T * S:
            raise _lib.MobocmfError("recommend_scores: moments has %d columns, not T S = %d" % (moments.shape[2], T * S))
        dev = moments.device
        if scale is not None:
            scale = _prep(torch.as_tensor(scale, dtype=torch.float64, device=dev))
            if tuple(scale.shape) != (moments.shape[0], 2):
                raise _lib.MobocmfError("recommend_scores: scale must be (n_obj + n_con, 2)")
        if F is None:
            F = _empty(max(n_obj, 0), max(T, 0), device=dev)
        elif F.dim() != 2 or F.shape[0] != n_obj or F.shape[1] < T or F.dtype != torch.float64 or F.device != dev \
                or (F.shape[1] > 1 and F.stride(1) != 1):
            raise _lib.MobocmfError("recommend_scores: F must be (n_obj, >= T) float64 with unit column stride")
        if viol is None and n_con > 0:
            viol = _empty(max(T, 0), device=dev)
        elif viol is not None and (viol.dim() != 1 or viol.numel() < T or viol.dtype != torch.float64 or viol.device != dev
                                   or not viol.is_contiguous()):
            raise _lib.MobocmfError("recommend_scores: viol must be a contiguous (>= T,) float64 tensor")
        ldf = F.shape[1] if F.shape[0] < 2 else F.stride(0)
        _lib.check(lib.mobocmf_recommend_scores(_ptr(moments), n_obj, n_con, T, S, _ptr(scale), float(p_min),
                                                recommend_z_min(p_min) if z_min is None else float(z_min), _ptr(F), ldf,
                                                _ptr(viol), _on(stream)), "mobocmf_recommend_scores")
    return F, viol


def pareto_mask(vals, con_mean=None, con_var=None, noise=None, p_min=0.999):
    """The recommendation rule of the reference's BO driver in one call (mobocmf_pareto_mask): ``vals`` (k, n) objective values
    (minimised), optionally ``con_mean`` / ``con_var`` (K_con, n) Gaussian constraint predictions and ``noise`` (K_con,) to
    subtract from their variances.  A row is feasible when Phi(m / sqrt(v - noise)) > p_min for every constraint; the mask
    keeps the feasible rows that MOOP.compute_pareto_front keeps among them (of equal rows the first).  Feasible rows with a NaN
    objective are never kept.  Returns (mask (n,) bool, counts (3,) int64 = feasible rows, front rows, feasible NaN rows), both
    on the device.  No autograd."""
    lib = _lib.require_device()
    with torch.no_grad():
        if vals.dim() != 2 or not 1 <= vals.shape[0] <= _lib.PARETO_MAX_K:
            raise _lib.MobocmfError("pareto_mask: vals must be (k, n) with 1 <= k <= %d" % _lib.PARETO_MAX_K)
        vals = _prep(vals.detach())
        k, n = vals.shape
        K_con = 0
        if con_mean is not None or con_var is not None:
            if con_mean is None or con_var is None or con_mean.dim() != 2 or tuple(con_mean.shape) != tuple(con_var.shape) \
                    or con_mean.shape[1] != n:
                raise _lib.MobocmfError("pareto_mask: con_mean and con_var must both be (K_con, n)")
            con_mean, con_var = _prep(con_mean.detach()), _prep(con_var.detach())
            K_con = con_mean.shape[0]
        if noise is not None:
            noise = _prep(torch.as_tensor(noise, dtype=torch.float64, device=vals.device).reshape(-1))
            if noise.numel() != K_con:
                raise _lib.MobocmfError("pareto_mask: noise needs one entry per constraint")
        mask = torch.empty(n, dtype=torch.int32, device=vals.device)
        counts = torch.empty(3, dtype=torch.int64, device=vals.device)
        _lib.check(lib.mobocmf_pareto_mask(k, n, _ptr(vals), max(n, 1), K_con, _ptr(con_mean), _ptr(con_var), max(n, 1),
                                           _ptr(noise), float(p_min), _ptr(mask), _ptr(counts), _stream()),
                   "mobocmf_pareto_mask")
    return mask.bool(), counts


def hypervolume(front, ref_point):
    """Exact hypervolume (mobocmf_hypervolume) of ``front`` (P, k) -- minimised objectives -- against ``ref_point`` (k,): the
    volume of the union of the boxes [p, ref] over the points that weakly dominate ref.  1 <= k <= 5, P within the bound of
    ``_lib.HV_MAX_POINTS``; NaN input and larger shapes raise.  Returns a Python float (synchronises); bitwise reproducible."""
    lib = _lib.require_device()
    with torch.no_grad():
        if front.dim() != 2 or not 1 <= front.shape[1] <= _lib.HV_MAX_K:
            raise _lib.MobocmfError("hypervolume: front must be (P, k) with 1 <= k <= %d" % _lib.HV_MAX_K)
        front = _prep(front.detach())
        P, k = front.shape
        ref = _prep(torch.as_tensor(ref_point, dtype=torch.float64).reshape(-1).to(front.device))
        if ref.numel() != k:
            raise _lib.MobocmfError("hypervolume: ref_point needs %d entries" % k)
        nb = _lib._SZ()
        _lib.check(lib.mobocmf_hypervolume_workspace_bytes(k, P, ctypes.byref(nb)),
                   "mobocmf_hypervolume_workspace_bytes (k = %d, P = %d; bound %d points)" % (k, P, _lib.HV_MAX_POINTS[k]))
        ws = scratch_buffer(nb.value, front.device)
        out = ctypes.c_double()
        _lib.check(lib.mobocmf_hypervolume(k, P, _ptr(front), k, _ptr(ref), ctypes.byref(out), _ptr(ws), nb.value, _stream()),
                   "mobocmf_hypervolume (NaN in the front or the reference point?)")
    return out.value


def select_inducing(x, hyp, max_points, tol_rel=0.0, form=None):
    """Inducing points by greedy conditional variance (mobocmf_select_inducing): the incomplete pivoted Cholesky of K_nn
    under the kind-0 kernel with ``hyp`` = [outputscale, lengthscales] (``hyp_len(0, d)`` entries).  Every step picks the row
    of ``x`` (N, d) with the largest residual diag(K_nn - K_nm K_mm^-1 K_mn) -- ties: the lowest row -- and stops after
    ``max_points`` picks or before a pick whose residual is <= ``tol_rel`` * outputscale.  ``form``: None = by size, 1 = the
    one-workgroup launch (N <= ``_lib.INDUCING_ONE_WG_MAX_ROWS``), 2 = one launch per pivot (bitwise the same result).
    Returns (idx [count] int64 in pick order, resid [count] the residual of each pick when it was picked, diag [N] the
    residuals left).  Synchronises once to read ``count``; non-finite ``x`` / ``hyp`` and non-positive hyper-parameters raise."""
    lib = _lib.require_device()
    with torch.no_grad():
        if x.dim() != 2 or not 1 <= x.shape[1] <= _lib.MAX_D:
            raise _lib.MobocmfError("select_inducing: x must be (N, d) with 1 <= d <= %d" % _lib.MAX_D)
        x = _prep(x.detach())
        N, d = x.shape
        hyp = _prep(torch.as_tensor(hyp, dtype=torch.float64).detach().reshape(-1).to(x.device))
        if hyp.numel() != hyp_len(0, d):
            raise _lib.MobocmfError("select_inducing: hyp needs %d entries (outputscale, then d lengthscales)" % hyp_len(0, d))
        max_points, form = int(max_points), 0 if form is None else int(form)
        nb = _lib._SZ()
        _lib.check(lib.mobocmf_select_inducing_workspace_bytes(N, max_points, ctypes.byref(nb)),
                   "mobocmf_select_inducing_workspace_bytes (N = %d, max_points = %d; 1 <= max_points <= min(N, %d), N <= %d)"
                   % (N, max_points, _lib.INDUCING_MAX_POINTS, _lib.INDUCING_MAX_ROWS))
        ws = scratch_buffer(nb.value, x.device)
        idx = _empty(max_points, dtype=torch.int32, device=x.device)
        head = _empty(2, dtype=torch.int32, device=x.device)           # count, info
        resid = _empty(max_points, device=x.device)
        diag = _empty(N, device=x.device)
        _lib.check(lib.mobocmf_select_inducing(N, d, _ptr(x), _ptr(hyp), max_points, float(tol_rel), form, _ptr(idx),
                                               ctypes.c_void_p(head.data_ptr()), _ptr(resid), _ptr(diag),
                                               ctypes.c_void_p(head.data_ptr() + 4), _ptr(ws), nb.value, _stream()),
                   "mobocmf_select_inducing (form 1 takes at most %d rows)" % _lib.INDUCING_ONE_WG_MAX_ROWS)
        count, info = (int(v) for v in head.tolist())
        if info != 0:
            raise _lib.MobocmfError("select_inducing refused its input: %s (info = %d)" % (_lib.INDUCING_INFO.get(info, "?"), info))
    return idx[:count].long(), resid[:count], diag


# ------------------------------------------------------------------------------------------------------------
# Mini-batches drawn on the device (csrc/minibatch.hip).  Thin wrappers: they only enqueue launches on the
# current stream and read nothing back, so a captured step may contain them.
# ------------------------------------------------------------------------------------------------------------
def minibatch_state(seed, device):
    """int64 [seed, step, status] of one sampler on ``device``: step counts the batches drawn, status is 0 or a sticky code
    of ``_lib.MINIBATCH_STATUS``.  The launches advance it on the device."""
    _lib.require_device()
    return torch.tensor([int(seed), 0, 0], dtype=torch.int64, device=device)


def _mb_i64(t, n, what):
    if not t.is_cuda or t.dtype != torch.int64 or not t.is_contiguous() or t.numel() < n:
        raise _lib.MobocmfError("mobocmf_amd: %s must be a contiguous int64 GPU tensor of at least %d entries" % (what, n))
    return t


def minibatch_indices(state, fid, batch_size, num_levels, src, counts, order_by_fidelity=True):
    """The next batch of the sampler ``state``: ``src[:rows]`` = its source rows (``rows = src.numel()`` is what the caller
    expects the batch to have: ``batch_size``, or the ragged rest for the last batch of an epoch), ordered stably by descending
    fidelity when asked; ``counts[l]`` = number of its rows with fidelity >= l.  Advances the step count.  If the batch does
    not have ``rows`` rows the launch only sets ``state[2]`` (see ``minibatch_check``)."""
    lib = _lib.require_device()
    fid = _prep(fid)
    N, rows = fid.numel(), src.numel()
    _mb_i64(state, 3, "state"), _mb_i64(src, 1, "src"), _mb_i64(counts, num_levels, "counts")
    _lib.check(lib.mobocmf_minibatch_indices(N, int(batch_size), int(num_levels), _ptr(fid), int(bool(order_by_fidelity)), rows,
                                             _ptr(state), _ptr(src), _ptr(counts), _stream()),
               "mobocmf_minibatch_indices (N = %d, batch_size = %d, levels = %d, rows = %d)" % (N, batch_size, num_levels, rows))


def minibatch_gather(state, src, x, y, fid, xb, yb, fidb):
    """xb[r] = x[src[r]], yb[r] = y[src[r]], fidb[r] = fid[src[r]] for the ``src.numel()`` rows of the batch (whole rows of
    ``x`` (N, d)); into caller-owned buffers."""
    lib = _lib.require_device()
    x, y, fid = _prep(x), _prep(y), _prep(fid)
    N, d = x.shape
    rows = src.numel()
    _mb_i64(state, 3, "state"), _mb_i64(src, 1, "src")
    for t, n, what in ((xb, rows * d, "xb"), (yb, rows, "yb"), (fidb, rows, "fidb")):
        if not t.is_cuda or t.dtype != torch.float64 or not t.is_contiguous() or t.numel() != n:
            raise _lib.MobocmfError("mobocmf_amd: %s must be a contiguous float64 GPU tensor of %d entries" % (what, n))
    if y.numel() != N or fid.numel() != N:
        raise _lib.MobocmfError("mobocmf_amd: minibatch_gather needs one y and one fidelity per row of x")
    _lib.check(lib.mobocmf_minibatch_gather(N, d, rows, _ptr(x), _ptr(y), _ptr(fid), _ptr(src), _ptr(state), _ptr(xb), _ptr(yb),
                                            _ptr(fidb), _stream()), "mobocmf_minibatch_gather (N = %d, d = %d)" % (N, d))


def minibatch_accumulate(state, num_data, batch_size, loss, kl, sums):
    """sums[0:2] += (loss, kl) of the step just taken (restarted at the first batch of an epoch); sums[2:4] = the sums of the
    last finished epoch."""
    lib = _lib.require_device()
    _lib.check(lib.mobocmf_minibatch_accumulate(int(num_data), int(batch_size), _ptr(state), _ptr(loss), _ptr(kl), _ptr(sums),
                                                _stream()), "mobocmf_minibatch_accumulate")


def minibatch_check(state):
    """Synchronising: raises if a launch of the sampler refused its batch (``state[2]`` set)."""
    status = int(state[2])
    if status != 0:
        raise FloatingPointError("mini-batch sampler: %s (status = %d)" % (_lib.MINIBATCH_STATUS.get(status, "?"), status))


def minibatch_permutation(seed, epoch, num_data):
    """Host-side: the source rows of positions 0..num_data-1 of ``epoch`` (int64 CPU tensor), from the definition the index
    launch uses -- which rows a step used, without asking the device.  Not a training path."""
    lib = _lib.load()
    out = torch.empty(int(num_data), dtype=torch.int64)
    _lib.check(lib.mobocmf_minibatch_permutation_host(int(seed), int(epoch), int(num_data), ctypes.c_void_p(out.data_ptr())),
               "mobocmf_minibatch_permutation_host")
    return out


# ------------------------------------------------------------------------------------------------------------
# Exact-GP comparison baselines on the layer's kernels: Gram (mobocmf_gram_forward), the multi-fidelity
# combination, the blocked Cholesky + triangular inverse of the chain, the triangular MFMA product with column statistics.
# Evaluation only (no autograd): fitting the baselines' hyper-parameters differentiates the plain-torch statement.
# ------------------------------------------------------------------------------------------------------------
def mf_kernel_combine(Ks, Kn, s1, s2, l1, l2, ntab, diag=0.0):
    """K[i][j] = s1[i] s2[j] Ks[i][j] + ntab[min(l1[i], l2[j])] Kn[i][j] (+ diag on the diagonal); l1 / l2 int32 levels."""
    lib = _lib.require_device()
    with torch.no_grad():
        Ks, Kn, s1, s2, ntab = (_prep(t) for t in (Ks, Kn, s1, s2, ntab))
        n1, n2 = Ks.shape
        if tuple(Kn.shape) != (n1, n2) or l1.numel() != n1 or l2.numel() != n2 or l1.dtype != torch.int32 or l2.dtype != torch.int32:
            raise _lib.MobocmfError("mf_kernel_combine: shape / dtype mismatch")
        if int(max(l1.max(), l2.max())) >= ntab.numel() or int(min(l1.min(), l2.min())) < 0:
            raise _lib.MobocmfError("mf_kernel_combine: fidelity level outside the noise-factor table")
        l1, l2 = l1.contiguous(), l2.contiguous()
        out = _empty(n1, n2, device=Ks.device)
        _lib.check(lib.mobocmf_mf_kernel_combine(n1, n2, _ptr(Ks), _ptr(Kn), Ks.stride(0), _ptr(s1), _ptr(s2), _ptr(l1), _ptr(l2),
                                                 _ptr(ntab), float(diag), _ptr(out), n2, n1, n2, _stream()),
                   "mobocmf_mf_kernel_combine")
    return out


class ExactGPState:
    """L, L^-1 and a = L^-1 y of an exact GP on n training points (mobocmf_exact_gp_factor)."""
    __slots__ = ("n", "state", "mll", "info")


def exact_gp_factor(K, y):
    """Factorises the n x n training covariance (noise on its diagonal); returns the state with ``.mll`` = log N(y | 0, K)
    and ``.info`` (0 or the failed pivot, device word)."""
    lib = _lib.require_device()
    with torch.no_grad():
        K, y = _prep(K), _prep(y.reshape(-1))
        n = K.shape[0]
        if K.shape[1] != n or y.numel() != n:
            raise _lib.MobocmfError("exact_gp_factor: K must be n x n and y of length n")
        sb, cb = ctypes.c_size_t(), ctypes.c_size_t()
        _lib.check(lib.mobocmf_exact_gp_workspace_bytes(n, 1, ctypes.byref(sb), ctypes.byref(cb)), "mobocmf_exact_gp_workspace_bytes")
        st = ExactGPState()
        st.n = n
        st.state = _poison(torch.empty(sb.value, dtype=torch.uint8, device=K.device))
        st.mll = _empty((), device=K.device)
        st.info = torch.zeros((), dtype=torch.int32, device=K.device)
        scratch = scratch_buffer(cb.value, K.device)
        _lib.check(lib.mobocmf_exact_gp_factor(n, _ptr(K), K.stride(0), _ptr(y), _ptr(st.mll), _ptr(st.info), _ptr(st.state),
                                               sb.value, _ptr(scratch), scratch.numel(), ctypes.byref(current_tuning()), _stream()),
                   "mobocmf_exact_gp_factor")
    return st


def _exact_state_views(st):
    """(L, L^-1, a = L^-1 y) of an ExactGPState as padded views (npad x npad, npad)."""
    npad = (st.n + 127) // 128 * 128
    buf = st.state.view(torch.float64)
    step = (npad * npad * 8 + 255) // 256 * 256 // 8
    vstep = (npad * 8 + 255) // 256 * 256 // 8
    L = buf[:npad * npad].view(npad, npad)
    Li = buf[step:step + npad * npad].view(npad, npad)
    a = buf[2 * step:2 * step + npad]
    del vstep
    return L, Li, a, npad


class _ExactGPMLL(torch.autograd.Function):
    """log N(y | 0, K) with its gradient, both on the library's kernels: forward = mobocmf_exact_gp_factor (blocked Cholesky,
    triangular inverse, a = L^-1 y, the likelihood), backward = d/dK = (alpha alpha^T - K^-1) / 2 with alpha = L^-T a and
    K^-1 = L^-T L^-1 as ONE triangular product on the f64 MFMA kernel, d/dy = -alpha.  What gpytorch's
    ExactMarginalLogLikelihood (x n) differentiates through torch.linalg (mfgp.py:63-64 of the reference fits through it)."""

    @staticmethod
    def forward(ctx, K, y):
        st = exact_gp_factor(K, y)
        ctx.st = st
        ctx.y_shape = y.shape
        return st.mll.clone()

    @staticmethod
    def backward(ctx, g):
        st = ctx.st
        n = st.n
        with torch.no_grad():
            _, Li, a, npad = _exact_state_views(st)
            LiT = Li.t().contiguous()
            Kinv = gemm_f64(LiT, LiT, trans_b=True, tri=2)          # L^-T (L^-T)^T, A upper triangular
            alpha = LiT @ a
            gK = (0.5 * g) * (torch.outer(alpha[:n], alpha[:n]) - Kinv[:n, :n])
            gy = (-g) * alpha[:n]
        return gK, gy.reshape(ctx.y_shape)


def exact_gp_mll(K, y):
    """Differentiable log N(y | 0, K) on the library's kernels (K: n x n incl. the noise on its diagonal).  The caller checks
    ``exact_gp_mll.last_info`` style failures through the returned value: a failed pivot makes the value NaN."""
    return _ExactGPMLL.apply(K, y)


def exact_gp_predict(st, Kts, kss):
    """Posterior mean and variance at the nt columns of Kts [n x nt] (prior variances kss)."""
    lib = _lib.require_device()
    with torch.no_grad():
        Kts, kss = _prep(Kts), _prep(kss.reshape(-1))
        n, nt = Kts.shape
        if n != st.n or kss.numel() != nt:
            raise _lib.MobocmfError("exact_gp_predict: shape mismatch")
        sb, cb = ctypes.c_size_t(), ctypes.c_size_t()
        _lib.check(lib.mobocmf_exact_gp_workspace_bytes(n, nt, ctypes.byref(sb), ctypes.byref(cb)), "mobocmf_exact_gp_workspace_bytes")
        scratch = scratch_buffer(cb.value, Kts.device)
        mean, var = _empty(nt, device=Kts.device), _empty(nt, device=Kts.device)
        _lib.check(lib.mobocmf_exact_gp_predict(n, nt, _ptr(Kts), Kts.stride(0), _ptr(kss), _ptr(mean), _ptr(var), _ptr(st.state),
                                                st.state.numel(), _ptr(scratch), scratch.numel(), ctypes.byref(current_tuning()),
                                                _stream()), "mobocmf_exact_gp_predict")
    return mean, var


class _SoftplusPackFn(torch.autograd.Function):
    """softplus of several raw parameter tensors, concatenated: one launch forward, one backward (mobocmf_softplus_pack)."""

    @staticmethod
    def forward(ctx, *raws):
        lib = _lib.require_device()
        flat = [_prep(r.detach().reshape(-1)) for r in raws]
        n = len(flat)
        sizes = (ctypes.c_int32 * n)(*[f.numel() for f in flat])
        ptrs = (ctypes.c_void_p * n)(*[f.data_ptr() for f in flat])
        out = _empty(sum(f.numel() for f in flat), device=flat[0].device)
        _lib.check(lib.mobocmf_softplus_pack(n, ptrs, sizes, _ptr(out), _stream()), "mobocmf_softplus_pack")
        ctx.save_for_backward(*raws)
        return out

    @staticmethod
    def backward(ctx, g):
        lib = _lib.require_device()
        raws = ctx.saved_tensors
        flat = [_prep(r.detach().reshape(-1)) for r in raws]
        n = len(flat)
        grads = [_empty_like(r) for r in raws]
        sizes = (ctypes.c_int32 * n)(*[f.numel() for f in flat])
        ptrs = (ctypes.c_void_p * n)(*[f.data_ptr() for f in flat])
        gptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in grads])
        _lib.check(lib.mobocmf_softplus_pack_backward(n, ptrs, sizes, _ptr(_prep(g)), gptrs, _stream()),
                   "mobocmf_softplus_pack_backward")
        return tuple(grads)


class _SoftplusPackSegFn(torch.autograd.Function):
    """``softplus_pack`` of the raw tensors of SEVERAL consumers (the layers of a model) in one launch: the packed vector is
    handed out as one tensor per consumer (``seg`` = raw tensors per consumer); the backward collects the consumers' gradients
    through a per-tensor pointer table -- one launch, no concatenation of gradients, no slice-backward launches."""

    @staticmethod
    def forward(ctx, seg, *raws):
        lib = _lib.require_device()
        flat = [_prep(r.detach().reshape(-1)) for r in raws]
        n = len(flat)
        sizes = (ctypes.c_int32 * n)(*[f.numel() for f in flat])
        ptrs = (ctypes.c_void_p * n)(*[f.data_ptr() for f in flat])
        out = _empty(sum(f.numel() for f in flat), device=flat[0].device)
        _lib.check(lib.mobocmf_softplus_pack(n, ptrs, sizes, _ptr(out), _stream()), "mobocmf_softplus_pack")
        ctx.save_for_backward(*raws)
        ctx.seg = tuple(seg)
        ctx.set_materialize_grads(False)
        outs, off, k = [], 0, 0
        for cnt in seg:
            ln = sum(f.numel() for f in flat[k:k + cnt])
            outs.append(out[off:off + ln])
            off, k = off + ln, k + cnt
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gs):
        lib = _lib.require_device()
        raws = ctx.saved_tensors
        flat = [_prep(r.detach().reshape(-1)) for r in raws]
        n = len(flat)
        grads = [_empty_like(r) for r in raws]
        sizes = (ctypes.c_int32 * n)(*[f.numel() for f in flat])
        ptrs = (ctypes.c_void_p * n)(*[f.data_ptr() for f in flat])
        gptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in grads])
        src, k, keep = [], 0, []
        for cnt, g in zip(ctx.seg, gs):
            g = None if g is None else _prep(g)
            keep.append(g)
            off = 0
            for f in flat[k:k + cnt]:
                src.append(0 if g is None else g.data_ptr() + 8 * off)
                off += f.numel()
            k += cnt
        _lib.check(lib.mobocmf_softplus_pack_backward_v(n, ptrs, sizes, (ctypes.c_void_p * n)(*src), gptrs, _stream()),
                   "mobocmf_softplus_pack_backward_v")
        return (None,) + tuple(grads)


def softplus_pack_segments(raw_groups):
    """One launch for several groups of raw tensors (<= 16 tensors in all): returns one packed, differentiable vector per group."""
    seg = [len(g) for g in raw_groups]
    return list(_SoftplusPackSegFn.apply(seg, *[r for g in raw_groups for r in g]))


def softplus_pack(raws):
    """``softplus(cat(raws))`` for float64 device tensors (<= 16 of them) in one launch, differentiable."""
    return _SoftplusPackFn.apply(*raws)


def syrk_weighted(A, w, H=None):
    """H = A diag(w) A^T (full symmetric, float64) on the k-sliced MFMA kernel: the weighted syrk of the layer backward
    (mobocmf_syrk_weighted_f64).  A: [Mr, Kd] with Mr, Kd multiples of 128."""
    lib = _lib.require_device()
    A, w = _prep(A), _prep(w)
    Mr, Kd = A.shape
    nb = _lib._SZ()
    snap = current_tuning()      # the size query and the launch: the same values
    _lib.check(lib.mobocmf_syrk_workspace_bytes(Mr, Kd, ctypes.byref(snap), ctypes.byref(nb)), "mobocmf_syrk_workspace_bytes")
    ws = scratch_buffer(nb.value, A.device)
    if H is None:
        H = _empty(Mr, Mr, device=A.device)
    _lib.check(lib.mobocmf_syrk_weighted_f64(Mr, Kd, _ptr(A), A.stride(0), _ptr(w), _ptr(H), _ptr(ws), nb.value,
                                             _ptr(getattr(_block_act_tls, "act", None)), ctypes.byref(snap), _stream()),
               "mobocmf_syrk_weighted_f64")
    return H


def gemm_f64(A, B, C=None, tri=0, trans_b=False, alpha=1.0, accumulate=False):
    """C (+)= alpha * A @ (B.T if trans_b else B) on the f64 MFMA kernel (tile-aligned shapes only)."""
    lib = _lib.require_device()
    A, B = _prep(A), _prep(B)
    Mr, Kd = A.shape
    Nc = B.shape[0] if trans_b else B.shape[1]
    if C is None:
        C = _empty(Mr, Nc, device=A.device)
    _lib.check(lib.mobocmf_gemm_f64(tri, int(trans_b), Mr, Nc, Kd, _ptr(A), A.stride(0), _ptr(B), B.stride(0), _ptr(C),
                                    C.stride(0), alpha, int(accumulate), ctypes.byref(current_tuning()), _stream()),
               "mobocmf_gemm_f64")
    return C
