"""What learnable inducing inputs cost and buy (GPU).  At C3's shape (d = 8, M = 512, N = 8192, S = 8) and at N = 65 536 / M = 512:

  step      the captured ELBO step's time with learn_inducing_locations off and on (one surrogate, mean of --steps replays back to back);
  kernels   mobocmf_gram_backward_rows next to mobocmf_gram_backward (g_x2 formed) on the layer-1 panel's shape M x N S and on
            the layer-0 panel's M x N, same inputs, same run; each call is its Gram kernel plus one reduction launch;
  quality   -ELBO after --epochs captured full-batch steps for `first` and `greedy_variance` initialisation, Z_x fixed
            against learned (fresh eps every step, lr 1e-2, the model's own initialisation heuristics).

One JSON line per figure on stdout.

    python tools/learn_inducing_bench.py [--shapes C3,N65536] [--steps 50] [--epochs 200] [--skip quality]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from mobocmf_amd import _lib                                   # noqa: E402
from mobocmf_amd.util import synthetic                         # noqa: E402

DEV = "cuda"
SHAPES = {"C3": dict(d=8, L=2, M=512, N=8192, S=8), "N65536": dict(d=8, L=2, M=512, N=65536, S=8)}


def _time(fn, n, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts), min(ts)


def _time_steps(g, n, warmup=3):
    """Microseconds per replay of a captured step: n replays back to back on the step's own stream, host clock around them."""
    for _ in range(warmup):
        g.step()
    g.stream.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        g.step()
    g.stream.synchronize()
    return (time.perf_counter() - t0) / n * 1e6


def step_times(name, cfg, steps):
    from mobocmf_amd.mlls import VariationalELBOMF
    from mobocmf_amd.util.graphed_step import GraphedELBOStep
    prob = synthetic.make_problem(seed=0, **cfg)
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64, device=DEV)
    out = {}
    for learn in (False, True):
        model = synthetic.model_from_problem(prob, device=DEV, **(dict(learn_inducing_locations=True) if learn else {}))
        g = GraphedELBOStep(model, VariationalELBOMF(model, cfg["N"], cfg["L"]), t(prob["x"]), t(prob["y"])[:, None],
                            t(prob["fid"])[:, None], lr=1e-3)
        out["learned" if learn else "fixed"] = _time_steps(g, steps)
        g.check()
        del g, model
        torch.cuda.empty_cache()
    print(json.dumps(dict(figure="step_us", shape=name, **cfg, fixed=round(out["fixed"], 1), learned=round(out["learned"], 1),
                          ratio=round(out["learned"] / out["fixed"], 4))), flush=True)


def kernel_times(name, cfg, steps):
    lib = _lib.require_device()
    d, M, S = cfg["d"], cfg["M"], cfg["S"]
    rng = np.random.default_rng(0)
    new = lambda *s: torch.as_tensor(rng.standard_normal(s), dtype=torch.float64, device=DEV)
    p = lambda x: ctypes.c_void_p(0 if x is None else x.data_ptr())
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for kind, xdiv in ((1, S), (0, 1)):
        nb = cfg["N"]
        Np = nb * xdiv
        x1, x2 = torch.rand(M, d, dtype=torch.float64, device=DEV), torch.rand(nb, d, dtype=torch.float64, device=DEV)
        f1, f2 = (new(M), new(Np)) if kind else (None, None)
        H = 5 + 2 * d if kind else 1 + d
        hyp = torch.cat([torch.full((H - (2 * d if kind else d),), 0.8, dtype=torch.float64), torch.full((2 * d if kind else d,), 0.7 * d ** 0.5, dtype=torch.float64)]).to(DEV)
        G = new(M, Np)
        nbytes, geo = ctypes.c_size_t(), (ctypes.c_int32 * 3)()
        _lib.check(lib.mobocmf_gram_backward_rows_workspace_bytes(kind, d, M, nb, xdiv, ctypes.byref(nbytes), geo), "rows size")
        ws = torch.empty(nbytes.value, dtype=torch.uint8, device=DEV)
        gz = torch.empty(M, d, dtype=torch.float64, device=DEV)
        rows = lambda: _lib.check(lib.mobocmf_gram_backward_rows(kind, d, p(x1), p(f1), M, p(x2), p(f2), nb, xdiv, p(hyp), p(G), Np, None,
                                                                 0, p(gz), p(ws), nbytes.value, stream()), "rows")
        nb2, geo2 = ctypes.c_size_t(), (ctypes.c_int32 * 3)()
        _lib.check(lib.mobocmf_gram_backward_workspace_bytes(kind, d, M, nb, xdiv, 1, ctypes.byref(nb2), geo2), "bwd size")
        ws2 = torch.empty(nb2.value, dtype=torch.uint8, device=DEV)
        gh, gf1, gf2, gx = (torch.empty(n, dtype=torch.float64, device=DEV) for n in (H, M, Np, nb * d))
        bwd = lambda: _lib.check(lib.mobocmf_gram_backward(kind, d, p(x1), p(f1), M, p(x2), p(f2), nb, xdiv, p(hyp), p(G), Np, None, None,
                                                           p(gh), p(gf1) if kind else None, p(gf2) if kind else None, p(gx), p(ws2),
                                                           nb2.value, stream()), "bwd")
        r_med, r_min = _time(rows, steps)
        b_med, b_min = _time(bwd, steps)
        print(json.dumps(dict(figure="gram_kernels_us", shape=name, kind=kind, M=M, columns=Np, xdiv=xdiv, d=d,
                              rows_call=round(r_med, 1), gram_backward_call=round(b_med, 1), ratio=round(r_med / b_med, 3),
                              rows_geometry=list(geo), gram_backward_geometry=list(geo2))), flush=True)
        del G, ws, ws2
        torch.cuda.empty_cache()


def quality(name, cfg, epochs):
    from mobocmf_amd.mlls import VariationalELBOMF
    from mobocmf_amd.models import MFDGP, TL
    from mobocmf_amd.util.graphed_step import GraphedELBOStep
    prob = synthetic.make_problem(seed=0, **cfg)
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64, device=DEV)
    x, y, fid = t(prob["x"]), t(prob["y"])[:, None], t(prob["fid"])[:, None]
    for sel in ("first", "greedy_variance"):
        res = {}
        for learn in (False, True):
            torch.manual_seed(0)
            model = MFDGP(x, y, fid, num_fidelities=cfg["L"], num_inducing=cfg["M"], inducing_selection=sel,
                          type_lengthscale=TL.MEDIAN if cfg["N"] <= 20000 else TL.ONES,      # the median needs n x n distances
                          num_samples_for_training=cfg["S"], inducing_device=DEV, learn_inducing_locations=learn).double().to(DEV)
            g = GraphedELBOStep(model, VariationalELBOMF(model, cfg["N"], cfg["L"]), x, y, fid, lr=1e-2)
            for _ in range(epochs):
                loss, _ = g.step()
            g.stream.synchronize()
            g.check()
            res["learned" if learn else "fixed"] = float(loss)
            del g, model
            torch.cuda.empty_cache()
        print(json.dumps(dict(figure="neg_elbo", shape=name, selection=sel, epochs=epochs, fixed=res["fixed"], learned=res["learned"],
                              ratio=round(res["learned"] / res["fixed"], 4))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="C3,N65536")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--epochs", type=int, default=200)
    ap.add_argument("--skip", default="", help="comma-separated: step, kernels, quality")
    args = ap.parse_args()
    skip = set(filter(None, args.skip.split(",")))
    for name in args.shapes.split(","):
        cfg = SHAPES[name]
        if "kernels" not in skip:
            kernel_times(name, cfg, args.steps)
        if "step" not in skip:
            step_times(name, cfg, args.steps)
        if "quality" not in skip:
            quality(name, cfg, args.epochs)


if __name__ == "__main__":
    main()
