#!/usr/bin/env python3
"""``BlackBoxMFDGPFitter.recommend(search="evolve")`` measured on surrogates of fixed parameters (util/synthetic.py, no training):
two objectives and one constraint, N = M = 64, S = 25 fixed samples, d in {2, 8}, population Np in {64, 128}.  The constraint is
shifted (``output_scaling``) so that a fifth of the 1000 d grid rows passes Phi(m / sqrt(v)) > 0.999.  Per (d, Np) one JSON line:

  * ``replay_us``: microseconds per generation of the captured graph replayed back to back (``--replays`` of them between two
    synchronisations, host clock);
  * ``launch_us`` / ``share``: microseconds per launch of a generation, each issued eagerly ``--replays`` times back to back in a
    run of its own (device events) -- vary, copy (the children into the group's x), forward (the predict group), scores
    (mobocmf_recommend_scores), survive (2 Np rows) -- and each one's share of their sum;
  * ``hv``: exact hypervolume of the grid's and of the evolved recommendation (``--generations`` generations) against a common
    reference point (max + 0.1 over both predicted fronts), and the rows of each;
  * ``empty_grid``: a 16-row grid made of rows the rule refuses -- the rows the grid mode returns (0) and the evolve mode returns.

usage: python tools/recommend_evolve_bench.py [--generations 100] [--replays 200] [--dims 2,8] [--pops 64,128]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mobocmf_amd import _lib  # noqa: E402
from mobocmf_amd import functional as F  # noqa: E402
from mobocmf_amd.mlls import VariationalELBOMF  # noqa: E402
from mobocmf_amd.util import synthetic  # noqa: E402
from mobocmf_amd.util.blackbox_mfdgp_fitter import BlackBoxMFDGPFitter, MFDGPHandler  # noqa: E402
from mobocmf_amd.util.hypervolume import HV  # noqa: E402
from mobocmf_amd.util.recommend_evolve import RecommendEvolve  # noqa: E402

DEV = "cuda"
NAMES = [("obj0", False), ("obj1", False), ("con0", True)]
P_MIN = 0.999


def make_fitter(d, N=64, M=64, S=25):
    fitter = BlackBoxMFDGPFitter(2, N, device=DEV)
    fitter.verbose = False
    for o, (name, is_con) in enumerate(NAMES):
        prob = synthetic.make_problem(d=d, L=2, M=M, N=N, S=S, output=o, seed=o)
        model = synthetic.model_from_problem(prob, device=DEV)
        h = MFDGPHandler.__new__(MFDGPHandler)
        h.mfdgp, h.num_data, h.num_fidelities, h.batch_size = model, N, 2, N
        h.global_index = 0 if is_con else o
        h.elbo = VariationalELBOMF(model, N, 2)
        h.iter_train_loader = None
        (fitter.mfdgp_handlers_cons if is_con else fitter.mfdgp_handlers_objs)[name] = h
        fitter.x_train = torch.as_tensor(prob["x"], dtype=torch.float64).to(DEV)
    fitter.num_obj, fitter.num_con = 2, 1
    fitter.thresholds_cons = torch.tensor([0.0], dtype=torch.float64)
    return fitter


def constraint_shift(fitter, grid, share=0.2):
    """(shift of the constraint's mean under which ``share`` of the grid rows is feasible, the margin z_min sd - mean per row)."""
    m = fitter.get_model("con0", True)
    with torch.no_grad():
        mu, v = m.predict_for_acquisition(torch.from_numpy(grid).to(DEV), 1)
        v = v.reshape(-1) - getattr(m, m.name_hidden_layer_likelihood + "1").noise.reshape(-1)[0]
    need = (F.recommend_z_min(P_MIN) * v.sqrt() - mu.reshape(-1)).cpu().numpy()
    return float(np.quantile(need, share)), need


def event_us(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return round(1e3 * a.elapsed_time(b) / n, 2)


def engine_times(fitter, scale, d, Np, replays):
    models = [fitter.get_model(name, con) for name, con in NAMES]
    eng = RecommendEvolve(models, 2, 1, Np, d, 1, p_min=P_MIN, scale=scale)
    eng.start(torch.rand(Np, d, dtype=torch.float64, generator=torch.Generator().manual_seed(Np)))
    eng.run(3)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(replays):
        eng._graph.replay()
    torch.cuda.synchronize()
    replay = round(1e6 * (time.perf_counter() - t0) / replays, 2)
    g = eng.group
    launch = {
        "vary": event_us(eng._vary, replays),
        "copy": event_us(lambda: g.x.copy_(eng.X[Np:]), replays),
        "forward": event_us(lambda: g._launch(_lib.STEP_FORWARD), replays),
        "scores": event_us(lambda: eng._scores(eng.F[:, Np:], 2 * Np, eng.viol[Np:]), replays),
        "survive": event_us(lambda: eng._survive(2 * Np, None), replays),
    }
    eng.finish()
    return replay, launch, type(g).__name__


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--generations", type=int, default=100)
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--dims", default="2,8")
    ap.add_argument("--pops", default="64,128")
    a = ap.parse_args()
    for d in [int(v) for v in a.dims.split(",")]:
        fitter = make_fitter(d)
        grid = np.random.default_rng((d, 1000)).random((1000 * d, d))
        shift, need = constraint_shift(fitter, grid)
        scaling = {"obj0": (0.0, 1.0), "obj1": (0.0, 1.0), "con0": (shift, 1.0)}
        scale = [list(scaling[name]) for name, _ in NAMES]
        refused = grid[np.flatnonzero(need > shift + 1e-9)[:16]]
        for Np in [int(v) for v in a.pops.split(",")]:
            replay, launch, engine = engine_times(fitter, scale, d, Np, a.replays)
            total = sum(launch.values())
            kw = dict(min_feasible_prob=P_MIN, output_scaling=scaling)
            _, gf, ginfo = fitter.recommend(grid, **kw)
            _, ef, einfo = fitter.recommend(grid, search="evolve", evolve_population=Np, evolve_generations=a.generations, **kw)
            hv = HV(ref_point=np.maximum(gf.max(0), ef.max(0)) + 0.1)
            e_grid = fitter.recommend(refused, **kw)[0]
            e_evolve = fitter.recommend(refused, search="evolve", evolve_population=16, evolve_generations=a.generations, **kw)[0]
            print(json.dumps({"d": d, "Np": Np, "engine": engine, "generations": a.generations, "replay_us": replay,
                              "launch_us": launch, "launch_sum_us": round(total, 2),
                              "share": {k: round(v / total, 3) for k, v in launch.items()},
                              "hv": {"grid": hv(gf), "evolve": hv(ef)},
                              "front_rows": {"grid": len(gf), "evolve": len(ef), "evolved": einfo["num_evolved"]},
                              "grid_feasible": ginfo["num_feasible"],
                              "empty_grid": {"grid_rows": len(e_grid), "evolve_rows": len(e_evolve)}}), flush=True)


if __name__ == "__main__":
    main()
