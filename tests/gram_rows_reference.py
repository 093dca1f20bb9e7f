"""Reference, summation depth and direct callers of the ROW-side Gram backward (gram_rows.hip, mobocmf_gram_backward_rows): the
gradient of L = sum G . K with respect to the row inputs x1 -- the inducing inputs Z_x.

The kernel function is symmetric in its arguments, so the row-side gradient of a case c = gram_case(kind, d, n1, nbase2, xdiv)
under G is the column-side gradient g_x2 of the TRANSPOSED case under G^T:

    x1' = repeat(x2, xdiv), f1' = f2;      x2' = x1, f2' = f1;      xdiv' = 1;      G' = G^T

and kernel_reference.gram_bwd_hp gives it together with its weights W and A (every addend of g_x1 is an addend of the
transposed case's g_x2, with the same exponent), so the bound |got - ref| <= 2^-53 (c W + D A) of kernel_reference, "Gram
backward", and its constant c = GRAM_BWD_C carry over; tests/test_gram_rows_cpu.py keeps that argument honest on these shapes.
Symmetric (K_mm) mode: both arguments are the same inputs, the reference is the row side plus the column side g_x2 of the
untransposed case."""
import ctypes

import numpy as np
import torch

from tests import kernel_reference as R

ROWS_N1 = (1, 31, 33, 65)             # straddle the 64-row group (and half of it)
ROWS_NBASE2 = (1, 127, 129, 257)      # straddle the 128-column activity block and the chunk edge
ROWS_XDIV = (1, 3, 8, 16)
ROWS_D_CASES = ((33, 129, 3), (65, 257, 8))
ROWS_D = (1, 2, 8, 9, 32)             # both edges of the 2- / 8- / 32-wide instantiations; 32 = MOBOCMF_MAX_D


def transposed_case(c, xdiv):
    return dict(x1=np.repeat(c["x2"], xdiv, axis=0), f1=c["f2"], x2=c["x1"], f2=c["f1"], hyp=c["hyp"])


def _masked(G, active):
    if active is None:
        return G
    return np.where(R.column_mask(active, G.shape[1])[None, :], G, 0.0)     # inactive blocks may hold NaN: exact zeros


def _rows(fn, kind, c, xdiv, G, active, symmetric):
    G = _masked(np.asarray(G), active)
    v, W, A = fn(kind, transposed_case(c, xdiv), 1, np.ascontiguousarray(G.T))["g_x2"]
    if symmetric:
        assert xdiv == 1 and c["x1"].shape == c["x2"].shape
        v2, W2, A2 = fn(kind, c, 1, G)["g_x2"]
        v, W, A = v + v2, W + W2, A + A2
    return {"g_x1": (v, W, A)}


def gram_rows_hp(kind, c, xdiv, G, active=None, symmetric=False):
    """{'g_x1': (gradient, W, A)} [n1 x d] in longdouble."""
    return _rows(R.gram_bwd_hp, kind, c, xdiv, G, active, symmetric)


def gram_rows_f64(kind, c, xdiv, G, active=None, symmetric=False):
    """The same statements in float64: the restatement behind GRAM_BWD_RATIO_MEASURED on these shapes."""
    return _rows(R.gram_bwd_f64, kind, c, xdiv, G, active, symmetric)


def symmetric_case(kind, d, n, seed=0):
    """A K_mm case: both sides hold the same inputs, G symmetric."""
    c = dict(R.gram_case(kind, d, n, n, 1, seed))
    c["x2"], c["f2"] = c["x1"], c["f1"]
    G, _ = R.gram_bwd_inputs(n, n, seed=seed + n)
    return c, G + G.T


def gram_rows_depth(geometry, xdiv, n1, d):
    """D of the bound: the roundings a partial sum holding a given addend can pass through, read off gram_bwd_rows_kernel and
    the reduction.  geometry = (column chunks, row groups, base columns per chunk); a wavefront owns wb = geometry[2] / 4 base
    columns and walks them in tiles = ceil(wb xdiv / 32) tiles of 32 columns.  Additions: the replica sums of a base column's
    part of a tile (Gsum; S1, S2, G2s): at most xdiv; nu zf S1 + af S2: 1; the thread's accumulators A1 / A2, one addition per
    base column and tile it shows up in: at most wb + tiles; A1 / ls1^2 + A2 / ls2^2: 1; the four wavefronts (w0 + w1) + (w2 +
    w3): 2; the reduction over the chunks (kernel_reference.sum_depth).  Products applied to a sum round it once more each --
    a1 E1 * (..), W * (x - z), * il^2, * 2 is exact: within kernel_reference.GRAM_BWD_MULS, added as there."""
    chunks, _, cb = geometry
    wb = cb // 4
    tiles = -(-wb * xdiv // 32)
    return {"g_x1": xdiv + 1 + wb + tiles + 1 + 2 + R.GRAM_BWD_MULS + R.sum_depth(chunks, n1 * d)}


def gram_rows_geometry(kind, d, n1, nbase2, xdiv):
    """(workspace bytes, (column chunks, row groups, base columns per chunk)): a host computation, no device needed."""
    from mobocmf_amd import _lib
    nb, geo = ctypes.c_size_t(), (ctypes.c_int32 * 3)()
    _lib.check(_lib.load().mobocmf_gram_backward_rows_workspace_bytes(kind, d, n1, nbase2, xdiv, ctypes.byref(nb), geo),
               "mobocmf_gram_backward_rows_workspace_bytes")
    return nb.value, tuple(geo)


class GramRows:
    """What gram_rows leaves behind: ``out`` {'g_x1': [n1 x d] float64 numpy}, ``geometry``, ``untouched`` (every guard double
    behind g_x1 and behind the workspace is still NaN), ``ws`` (the workspace, as the call left it)."""


def gram_rows(kind, d, x1, f1, n1, x2, f2, nbase2, xdiv, hyp, G, ldk, colact=None, symmetric=0, guard=8, ws_bytes=None,
              check=True, g_x1="new", ws="new"):
    """mobocmf_gram_backward_rows with the pointers as given: g_x1 and a workspace of exactly the reported size (``ws_bytes``:
    that size is passed instead) NaN before the call, ``guard`` NaN doubles behind each.  Returns a GramRows, or the status if
    ``check`` is False and the call is refused (then g_x1 and the workspace must still be all NaN: asserted here)."""
    from mobocmf_amd import _lib
    try:
        nbytes, geo = gram_rows_geometry(kind, d, n1, nbase2, xdiv)
    except _lib.MobocmfError:
        if check:
            raise
        nbytes, geo = 4096, None      # a shape the size query refuses: the call must refuse it too, whatever it is given
    assert nbytes % 8 == 0
    new = lambda n: torch.full((n + guard,), R.NAN, dtype=torch.float64, device="cuda")
    out = new(n1 * d) if isinstance(g_x1, str) else g_x1
    use = nbytes if ws_bytes is None else ws_bytes
    wsb = new(max(nbytes, use) // 8) if isinstance(ws, str) else ws
    rc = R.lib().mobocmf_gram_backward_rows(kind, d, R._p(x1), R._p(f1), n1, R._p(x2), R._p(f2), nbase2, xdiv, R._p(hyp), R._p(G), ldk,
                                            R._p(colact), symmetric, R._p(out), R._p(wsb), use, R._stream())
    if not check and rc != 0:
        torch.cuda.synchronize()
        assert out is None or bool(torch.isnan(out).all()), "a refused call wrote g_x1"
        assert wsb is None or bool(torch.isnan(wsb).all()), "a refused call wrote the workspace"
        return rc
    _lib.check(rc, "mobocmf_gram_backward_rows")
    r = GramRows()
    r.geometry, r.ws = geo, wsb
    r.out = {"g_x1": out[:n1 * d].cpu().numpy().reshape(n1, d)}
    used = geo[0] * n1 * d
    r.untouched = bool(torch.isnan(out[n1 * d:]).all()) and bool(torch.isnan(wsb[used:]).all())
    assert (used * 8 + 255) // 256 * 256 == nbytes, (used, nbytes)
    return r
