"""Step time of the captured mini-batch step (GraphedMiniBatchStep: the batch drawn, ordered and gathered on the device inside the
HIP graph) against the host-loader path it replaces, the full-batch captured step and itself without the fidelity ordering.

  python tools/minibatch_bench.py --N 8192 --M 512 --B 512 2048            # C3's shape, 3 surrogates
  python tools/minibatch_bench.py --N 65536 --M 512 --B 4096
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/minibatch_bench.py --N 8192 --B 2048 --only captured   # sampler launches

Variants, all on the same surrogates' shapes, `--surrogates` of them side by side:
  captured    GraphedMiniBatchStep, order_by_fidelity=True, the surrogates in lockstep on their streams (what train_mfdgps() runs)
  unordered   the same with order_by_fidelity=False (what the ordering buys: the block skipping of the layer backward)
  loader      BlackBoxMFDGPFitter.update_model over DataLoader(shuffle=True), eager launches, one surrogate after the other
              (what train_mfdgps() ran for batch_size < N before, and still runs with use_graphs=False), as the fitter runs it:
              FusedAdam, the models' default host-checked Cholesky
  full        GraphedELBOStep on all N rows (one step = one epoch)
One "step" is one step of EVERY surrogate.  Each repeat times whole epochs of every variant in turn (alternating), ending in a
device synchronise; after each window (outside the timed region) every step object's check() is called, and the figure is the
median, over the windows that ended in a verified state, of the milliseconds per step.  One JSON line per (B, variant)."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=8192)
    ap.add_argument("--M", type=int, default=512)
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--S", type=int, default=8)
    ap.add_argument("--L", type=int, default=2)
    ap.add_argument("--B", type=int, nargs="+", default=[512, 2048])
    ap.add_argument("--surrogates", type=int, default=3)
    ap.add_argument("--steps", type=int, default=32, help="mini-batch steps per timed window (rounded up to whole epochs)")
    ap.add_argument("--full-steps", type=int, default=8, help="full-batch steps per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", nargs="+", default=["captured", "unordered", "loader", "full"])
    ap.add_argument("--lr", type=float, default=1e-5,
                    help="small on purpose: the windows time hundreds of steps on synthetic surrogates, and at 1e-3 these drift "
                         "until a K_mm fails its Cholesky (a failed one-launch factorisation costs its 1 s wait bound per step)")
    ap.add_argument("--potrf-cols", type=int, default=None,
                    help="functional.set_potrf_cols: 4 = the blocked Cholesky as a launch pair per 64 columns instead of one launch")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()

    from torch.utils.data import DataLoader, TensorDataset

    from mobocmf_amd import functional as F
    from mobocmf_amd.mlls import VariationalELBOMF
    from mobocmf_amd.util import synthetic
    from mobocmf_amd.util.blackbox_mfdgp_fitter import BlackBoxMFDGPFitter
    from mobocmf_amd.util.graphed_step import GraphedELBOStep, GraphedMiniBatchStep

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    if a.potrf_cols is not None:
        F.set_potrf_cols(a.potrf_cols)
    streams = [torch.cuda.Stream(device=dev) for _ in range(a.surrogates)]      # shared by every variant, as the fitter's pool
    t = lambda v: torch.as_tensor(np.asarray(v), dtype=torch.float64, device=dev)
    probs = [synthetic.make_problem(d=a.d, L=a.L, M=a.M, N=a.N, S=a.S, output=k % 3, seed=k) for k in range(a.surrogates)]
    perm = np.random.default_rng(1).permutation(a.N)                             # fidelities interleaved, as real data
    data = [(t(p["x"][perm]), t(p["y"][perm])[:, None], t(p["fid"][perm])[:, None]) for p in probs]

    def models():
        ms = [synthetic.model_from_problem(p, num_samples_for_training=a.S, device=dev) for p in probs]
        return ms, [VariationalELBOMF(m, a.N, a.L) for m in ms]

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(line + "\n")

    def lockstep(steps_objs, n):
        for _ in range(n):
            for g in steps_objs:
                g.step()

    full = None
    if "full" in a.only:                 # first: the largest scratch arena, so that the later captures fit into it
        ms, es = models()
        full = [GraphedELBOStep(m, e, x, y, f, lr=a.lr, stream=s) for m, e, (x, y, f), s in zip(ms, es, data, streams)]
    for B in a.B:
        nb = -(-a.N // B)
        epochs = max(1, -(-a.steps // nb))
        n_steps = epochs * nb
        runs = {}
        if "captured" in a.only or "unordered" in a.only:
            for name, ordered in (("captured", True), ("unordered", False)):
                if name not in a.only:
                    continue
                ms, es = models()
                gs = [GraphedMiniBatchStep(m, e, x, y, f, B, lr=a.lr, stream=s, order_by_fidelity=ordered,
                                           sampler_state=F.minibatch_state(100 + k, dev))
                      for k, (m, e, (x, y, f), s) in enumerate(zip(ms, es, data, streams))]
                runs[name] = (lambda gs=gs: lockstep(gs, n_steps), n_steps, gs)
        if "loader" in a.only:
            ms, es = models()
            opts = [F.FusedAdam(list(m.parameters()), lr=a.lr) for m in ms]
            loaders = [DataLoader(TensorDataset(x, y, f), batch_size=B, shuffle=True) for (x, y, f) in data]

            def run_loader(ms=ms, es=es, opts=opts, loaders=loaders):
                for _ in range(epochs):
                    for m, e, o, ld in zip(ms, es, opts, loaders):
                        BlackBoxMFDGPFitter.update_model(m, e, o, ld)
            runs["loader"] = (run_loader, n_steps, None)
        if full is not None:
            runs["full"] = (lambda: lockstep(full, a.full_steps), a.full_steps, full)
        for fn, _, _ in runs.values():   # every shape of every variant once before the timed windows
            fn()
        torch.cuda.synchronize()
        def verdict(gs):              # the state a window ended in (synchronising; outside the timed region)
            if gs is None:
                return True
            try:
                for g in gs:
                    g.check()
            except Exception as err:      # NotPSDError / FloatingPointError / an abandoned in-launch wait
                return "%s: %s" % (type(err).__name__, str(err)[:80])
            return True

        times = {k: [] for k in runs}
        oks = {k: [] for k in runs}
        for _ in range(a.repeats):
            for name, (fn, n, gs) in runs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e3 / n)
                oks[name].append(verdict(gs))
        for name, (fn, n, gs) in runs.items():
            good = [t for t, ok in zip(times[name], oks[name]) if ok is True]      # only windows that ended in a verified state count
            med = statistics.median(good) if good else None
            emit(dict(variant=name, N=a.N, M=a.M, d=a.d, S=a.S, L=a.L, B=(a.N if name == "full" else B), surrogates=a.surrogates,
                      steps_per_window=n, ms_per_step=med, ms_per_step_all=[round(v, 4) for v in times[name]],
                      ms_per_epoch=None if med is None else med * (1 if name == "full" else nb), windows_counted=len(good),
                      window_state=[ok if ok is True else ok for ok in oks[name]], potrf_cols=a.potrf_cols))
        for name, (_, _, gs) in runs.items():
            if gs is not None and name != "full":
                for g in gs:
                    g.retire()
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
