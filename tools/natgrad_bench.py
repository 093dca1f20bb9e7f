"""Natural gradients for q(u) (variational_optimizer="natgrad") against the default Adam step, on the layer path.

  python tools/natgrad_bench.py                       # C1, C2, C3 and the conditioned fit at N = M = 64
  python tools/natgrad_bench.py --configs C2 --epochs 100 300 --no-conditioned

Per configuration (one surrogate of synthetic.CONFIGS' shape, captured GraphedELBOStep, every parameter trained as in the second
training phase), both optimisers from the same initial state and the same fixed eps:
  time         ms per captured step, the two variants alternating in windows of --steps replays, median over --repeats windows
               that ended in a verified state (tiny learning rates: the timed windows must not drift into a failed Cholesky);
               a skipped step costs what a written one does, and the record says how many of the timed steps were skipped;
  convergence  -ELBO as the step reports it at epochs --epochs (the loss the k-th step evaluated, i.e. after k - 1
               updates), check() called at each of them; a failed verdict ends that variant's trajectory and is recorded.
Conditioned fit: two objectives and a constraint with N = M = 64, an injected Pareto set and fixed x~; the joint loss at iterations
--iters for both optimisers.  One JSON line per record; --out appends them to a file."""
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
    ap.add_argument("--configs", nargs="+", default=["C1", "C2", "C3"])
    ap.add_argument("--epochs", type=int, nargs="+", default=[100, 300, 1000, 3000])
    ap.add_argument("--iters", type=int, nargs="+", default=[50, 200, 2000])
    ap.add_argument("--lr", type=float, default=1e-3, help="Adam's learning rate (the fitter's lr_2)")
    ap.add_argument("--gamma", type=float, default=0.1)
    ap.add_argument("--gamma-init", type=float, default=1e-4)
    ap.add_argument("--warmup-steps", type=int, default=100)
    ap.add_argument("--steps", type=int, default=50, help="replays per timed window")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--no-conditioned", action="store_true")
    ap.add_argument("--no-time", action="store_true")
    ap.add_argument("--potrf-cols", type=int, default=None,
                    help="functional.set_potrf_cols: 4 = the blocked Cholesky as a launch pair per 64 columns instead of one launch")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from mobocmf_amd.mlls import VariationalELBOMF
    from mobocmf_amd.util import synthetic
    from mobocmf_amd.util.graphed_step import GraphedConditionedStep, GraphedELBOStep

    dev = torch.device("cuda:0")
    if a.potrf_cols is not None:
        from mobocmf_amd import functional as F
        F.set_potrf_cols(a.potrf_cols)
    t = lambda v: torch.as_tensor(np.asarray(v), dtype=torch.float64, device=dev)
    ng = dict(variational_optimizer="natgrad", natgrad_gamma=a.gamma, natgrad_gamma_init=a.gamma_init,
              natgrad_warmup_steps=a.warmup_steps)
    variants = (("adam", {}), ("natgrad", ng))

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(line + "\n")

    def verdict(step):
        try:
            step.check()
        except Exception as err:      # NotPSDError / FloatingPointError / an abandoned in-launch wait
            return "%s: %s" % (type(err).__name__, str(err)[:80])
        return True

    def trajectory(step, marks, what):
        out, done, ok = {}, 0, True
        for k in sorted(marks):
            for _ in range(k - done):
                step.step()
            done = k
            ok = verdict(step)
            if ok is not True:
                out[str(k)] = ok
                break
            out[str(k)] = float(step.loss)
        return dict(what, values=out, skipped=sum(step.skipped_steps()) if ok is True else None)

    for name in a.configs:
        cfg = {k: v for k, v in synthetic.CONFIGS[name].items() if k != "outputs"}
        prob = synthetic.make_problem(**cfg, seed=0)
        x, y, fid = t(prob["x"]), t(prob["y"])[:, None], t(prob["fid"])[:, None]
        eps = [None] + [t(e) for e in prob["eps"][1:]]

        def make(kw, lr):
            model = synthetic.model_from_problem(prob, num_samples_for_training=cfg["S"], device=dev)
            model.fix_variational_hypers(False)
            return GraphedELBOStep(model, VariationalELBOMF(model, cfg["N"], cfg["L"]), x, y, fid, lr=lr, fixed_eps=eps, **kw)

        if not a.no_time:
            tiny = dict(ng, natgrad_gamma=1e-6, natgrad_gamma_init=1e-6)
            steps = {"adam": make({}, 1e-6), "natgrad": make(tiny, 1e-6)}
            times = {k: [] for k in steps}
            failed = {k: [] for k in steps}      # verdicts of the windows that did not count
            for g in steps.values():
                for _ in range(5):
                    g.step()
            torch.cuda.synchronize()
            for _ in range(a.repeats):
                for k, g in steps.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(a.steps):
                        g.step()
                    torch.cuda.synchronize()
                    dt = (time.perf_counter() - t0) * 1e3 / a.steps
                    ok = verdict(g)
                    if ok is True:
                        times[k].append(dt)
                    else:
                        failed[k].append(ok)
            emit(dict(record="time", config=name, **cfg, steps_per_window=a.steps,
                      ms_per_step={k: (statistics.median(v) if v else None) for k, v in times.items()},
                      ms_per_step_all={k: [round(u, 4) for u in v] for k, v in times.items()},
                      windows_not_counted=failed, potrf_cols=a.potrf_cols,
                      skipped_in_timed_windows=sum(steps["natgrad"].optimizer.skipped.tolist())))
            for g in steps.values():
                g.close()
        for vname, kw in variants:
            g = make(kw, a.lr)
            emit(trajectory(g, a.epochs, dict(record="convergence", config=name, **cfg, optimizer=vname, lr=a.lr, gamma=a.gamma,
                                              gamma_init=a.gamma_init, warmup_steps=a.warmup_steps)))
            g.close()

    if not a.no_conditioned:
        from torch.utils.data import TensorDataset

        from mobocmf_amd.util.blackbox_mfdgp_fitter import BlackBoxMFDGPFitter, MFDGPHandler
        N = M = 64
        gen = torch.Generator().manual_seed(2)
        ps = torch.rand(10, 2, dtype=torch.float64, generator=gen)
        pf = torch.randn(10, 2, dtype=torch.float64, generator=gen) * 0.3
        xt = torch.rand(10, 2, dtype=torch.float64, generator=gen).to(dev)
        for vname, kw in variants:
            fitter = BlackBoxMFDGPFitter(2, N, device="cuda:0")
            fitter.verbose = False
            for o in range(3):
                prob = synthetic.make_problem(d=2, L=2, M=M, N=N, S=1, output=o, seed=o)
                prob["noise"] = [np.array(1e-2), np.array(2e-2)]
                model = synthetic.model_from_problem(prob, num_samples_for_training=1, device=dev)
                h = MFDGPHandler.__new__(MFDGPHandler)
                h.mfdgp, h.num_data, h.num_fidelities, h.batch_size = model, N, 2, N
                h.elbo = VariationalELBOMF(model, N, 2)
                h.train_dataset = TensorDataset(t(prob["x"]), t(prob["y"])[:, None], t(prob["fid"])[:, None])
                h.iter_train_loader = None
                (fitter.mfdgp_handlers_objs if o < 2 else fitter.mfdgp_handlers_cons)["bb%d" % o] = h
                model.fix_variational_hypers_cond(True)
            fitter.num_obj, fitter.num_con = 2, 1
            fitter.thresholds_cons = torch.tensor([0.1], dtype=torch.float64)
            fitter.set_pareto_solution(ps, pf)
            torch.manual_seed(0)
            g = GraphedConditionedStep(fitter, lr=a.lr, fixed_x_tilde=xt, **kw)
            emit(trajectory(g, a.iters, dict(record="conditioned", N=N, M=M, optimizer=vname, lr=a.lr, gamma=a.gamma,
                                             gamma_init=a.gamma_init, warmup_steps=a.warmup_steps)))
            g.close()
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
