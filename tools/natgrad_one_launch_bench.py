"""What natural gradients for q(u) cost per step at the sizes of the one-launch steps (M <= 128), three variants in one process:

  adam_one_launch     Adam through the one-launch step (TinyELBOStep where the surrogate fits it, CoopELBOStep otherwise)
  natgrad_layer_path  natural gradients in the captured layer-path step (GraphedELBOStep / GraphedConditionedStep)
  natgrad_one_launch  natural gradients through the one-launch step: its launch + ONE mobocmf_natgrad_small_step launch

  python tools/natgrad_one_launch_bench.py                       # C1, C2 and the conditioned fit at N = M = 64
  python tools/natgrad_one_launch_bench.py --configs C2 --no-conditioned

Per shape: one surrogate of synthetic.CONFIGS' shape (the conditioned fit: two objectives and a constraint, an injected Pareto
set, fixed x~), every variant from the same initial state; ms per step, the variants alternating in windows of --steps steps,
median over --repeats windows that ended in a verified state (tiny learning rates and gamma: the timed windows must not drift
into a failed Cholesky).  One JSON line per shape; --out appends them to a file."""
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
    ap.add_argument("--configs", nargs="+", default=["C1", "C2"])
    ap.add_argument("--steps", type=int, default=50, help="steps per timed window")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--no-conditioned", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from mobocmf_amd.mlls import VariationalELBOMF
    from mobocmf_amd.util import coop_step, synthetic, tiny_step
    from mobocmf_amd.util.graphed_step import GraphedConditionedStep, GraphedELBOStep

    dev = torch.device("cuda:0")
    t = lambda v: torch.as_tensor(np.asarray(v), dtype=torch.float64, device=dev)
    ng = dict(variational_optimizer="natgrad", natgrad_gamma=1e-6, natgrad_gamma_init=1e-6, natgrad_warmup_steps=100)
    lr = 1e-6

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

    def timed(steps, what):
        times, failed = {k: [] for k in steps}, {k: [] for k in steps}
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
                (times[k].append(dt) if ok is True else failed[k].append(ok))
        med = {k: (statistics.median(v) if v else None) for k, v in times.items()}
        ratio = lambda p, q: (med[p] / med[q] if med[p] and med[q] else None)
        emit(dict(what, steps_per_window=a.steps, ms_per_step=med, ms_per_step_all={k: [round(u, 4) for u in v] for k, v in times.items()},
                  one_launch_natgrad_over_layer_path=ratio("natgrad_one_launch", "natgrad_layer_path"),
                  one_launch_natgrad_over_adam=ratio("natgrad_one_launch", "adam_one_launch"), windows_not_counted=failed,
                  skipped={k: sum(g.skipped_steps()) for k, g in steps.items() if k != "adam_one_launch"}))
        for g in steps.values():
            g.close()

    for name in a.configs:
        cfg = {k: v for k, v in synthetic.CONFIGS[name].items() if k != "outputs"}
        prob = synthetic.make_problem(**cfg, seed=0)
        x, y, fid = t(prob["x"]), t(prob["y"])[:, None], t(prob["fid"])[:, None]
        eps = [None] + [t(e) for e in prob["eps"][1:]]

        def model():
            mdl = synthetic.model_from_problem(prob, num_samples_for_training=cfg["S"], device=dev)
            mdl.fix_variational_hypers(False)
            return mdl

        probe = model()
        cls = tiny_step.TinyELBOStep if tiny_step.eligible(probe, x, fid) else coop_step.CoopELBOStep
        one = lambda kw: cls([model()], [cfg["N"]], [x], [y], [fid], lr=lr, fixed_eps=[eps], **kw)
        mdl = model()
        steps = {"adam_one_launch": one({}),
                 "natgrad_layer_path": GraphedELBOStep(mdl, VariationalELBOMF(mdl, cfg["N"], cfg["L"]), x, y, fid, lr=lr,
                                                       fixed_eps=eps, **ng),
                 "natgrad_one_launch": one(ng)}
        timed(steps, dict(record="time", config=name, one_launch_class=cls.__name__, **cfg))

    if not a.no_conditioned:
        from torch.utils.data import TensorDataset

        from mobocmf_amd.util.blackbox_mfdgp_fitter import BlackBoxMFDGPFitter, MFDGPHandler
        N = M = 64
        gen = torch.Generator().manual_seed(2)
        ps = torch.rand(10, 2, dtype=torch.float64, generator=gen)
        pf = torch.randn(10, 2, dtype=torch.float64, generator=gen) * 0.3
        xt = torch.rand(10, 2, dtype=torch.float64, generator=gen).to(dev)

        def fitter():
            f = BlackBoxMFDGPFitter(2, N, device="cuda:0")
            f.verbose = False
            for o in range(3):
                prob = synthetic.make_problem(d=2, L=2, M=M, N=N, S=1, output=o, seed=o)
                prob["noise"] = [np.array(1e-2), np.array(2e-2)]
                mdl = synthetic.model_from_problem(prob, num_samples_for_training=1, device=dev)
                h = MFDGPHandler.__new__(MFDGPHandler)
                h.mfdgp, h.num_data, h.num_fidelities, h.batch_size = mdl, N, 2, N
                h.elbo = VariationalELBOMF(mdl, N, 2)
                h.train_dataset = TensorDataset(t(prob["x"]), t(prob["y"])[:, None], t(prob["fid"])[:, None])
                h.iter_train_loader = None
                (f.mfdgp_handlers_objs if o < 2 else f.mfdgp_handlers_cons)["bb%d" % o] = h
                mdl.fix_variational_hypers_cond(True)
            f.num_obj, f.num_con = 2, 1
            f.thresholds_cons = torch.tensor([0.1], dtype=torch.float64)
            f.set_pareto_solution(ps, pf)
            return f

        steps = {"adam_one_launch": coop_step.CoopConditionedStep(fitter(), lr=lr, fixed_x_tilde=xt),
                 "natgrad_layer_path": GraphedConditionedStep(fitter(), lr=lr, fixed_x_tilde=xt, **ng),
                 "natgrad_one_launch": coop_step.CoopConditionedStep(fitter(), lr=lr, fixed_x_tilde=xt, **ng)}
        timed(steps, dict(record="time", config="conditioned", one_launch_class="CoopConditionedStep", N=N, M=M))
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
