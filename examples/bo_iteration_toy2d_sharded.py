#!/usr/bin/env python3
"""One BO iteration of the toy 2-D problem of bo_iteration_toy2d.py with its black-boxes sharded over the ranks of a
process group (mobocmf_amd.parallel: one process per GPU, round-robin ownership): every rank fits its own surrogates, the
ranks draw one joint Pareto solution of ALL black-boxes (the packed posterior samples are exchanged, the same seeded MOOP
runs everywhere), fit the conditioned surrogates with the omega factors exchanged, and search the coupled acquisition
summed over the ranks.  Every rank prints its candidate and fidelity; they agree.

    python examples/bo_iteration_toy2d_sharded.py --ranks 2                   # one rank per GPU, RCCL
    python examples/bo_iteration_toy2d_sharded.py --ranks 2 --backend gloo    # two ranks on one card (RCCL refuses that)

Under an existing process group (``torch.distributed.run`` or ``parallel.launch_ranks`` environment), ``run()`` uses it.
"""
import argparse
import faulthandler
import os
import sys
import time

import numpy as np

faulthandler.enable()
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bo_iteration_toy2d import blackboxes  # noqa: E402
from mobocmf_amd import parallel  # noqa: E402
from mobocmf_amd.acquisition_functions.JESMOC_MFDGP import JESMOC_MFDGP  # noqa: E402
from mobocmf_amd.models.mfdgp import TL  # noqa: E402
from mobocmf_amd.util.blackbox_mfdgp_fitter import BlackBoxMFDGPFitter  # noqa: E402


def run(epochs=300, cond_iters=200, acq_iters=50, n_low=14, n_high=6, grid=100, seed=0, device="cuda", verbose=True):
    """One iteration on this rank's share of the black-boxes.  Returns (fitter, acquisition, candidate, fidelity)."""
    rank, world = parallel.world()
    rng = np.random.default_rng(seed)            # the same data on every rank
    torch.manual_seed(seed)
    np.random.seed(seed)
    x = rng.uniform(size=(n_low + n_high, 2))
    fid = np.concatenate([np.zeros(n_low), np.ones(n_high)])
    bbs = blackboxes()
    mine, _ = parallel.shard_blackboxes(list(bbs))
    obj_names = [n for n, (_, _, c) in bbs.items() if not c]
    con_names = [n for n, (_, _, c) in bbs.items() if c]
    fitter = BlackBoxMFDGPFitter(2, x.shape[0], num_epochs_1=epochs, num_epochs_2=epochs, pareto_set_size=10,
                                 opt_grid_size=grid, type_lengthscale=TL.MEDIAN, device=device)
    fitter.verbose = False
    for name in mine:
        lo, hi, is_con = bbs[name]
        y = np.where(fid == 0, lo(x), hi(x))
        gi = (con_names if is_con else obj_names).index(name)
        fitter.initialize_mfdgp(torch.from_numpy(x), torch.from_numpy(y)[:, None], torch.from_numpy(fid)[:, None], name,
                                is_constraint=is_con, global_index=gi)
    if fitter.x_train is None:            # a rank without black-boxes still takes part in every exchange
        fitter.x_train = torch.from_numpy(x)
    fitter.set_global_constraint_thresholds([0.0] * len(con_names))
    t = [time.perf_counter()]
    fitter.train_mfdgps()
    torch.cuda.synchronize(); t.append(time.perf_counter())
    fitter.num_epochs_2 = cond_iters
    # JESMOC_MFDGP samples the Pareto solution itself (argument-less call: rank 0 draws the seed and broadcasts it)
    acq = JESMOC_MFDGP(model=fitter, num_fidelities=2,
                       standard_bounds=torch.tensor([[0.0, 0.0], [1.0, 1.0]], dtype=torch.float64, device=device))
    torch.cuda.synchronize(); t.append(time.perf_counter())
    for f in range(2):
        for name, (_, _, is_con) in bbs.items():          # every black-box: the cost totals must agree over the ranks
            acq.add_blackbox(f, name, cost_evaluation=1.0 if f == 0 else 10.0, is_constraint=is_con)
    cand, fidelity = acq.get_nextpoint_coupled(iteration=0, verbose=False, maxiter=acq_iters)
    torch.cuda.synchronize(); t.append(time.perf_counter())
    if verbose:
        print("rank %d/%d holds %s: pareto set %s, front %s; seconds: fit %.2f | pareto sample + conditioned fit %.2f | "
              "acquisition search %.2f; next point %s at fidelity %d" %
              (rank, world, mine, tuple(fitter.pareto_set.shape), tuple(fitter.pareto_front.shape),
               t[1] - t[0], t[2] - t[1], t[3] - t[2], np.round(cand.cpu().numpy(), 6), fidelity))
        sys.stdout.flush()
    return fitter, acq, cand, fidelity


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ranks", type=int, default=2, help="ranks to start when not already inside a process group")
    ap.add_argument("--backend", choices=["nccl", "gloo"], default="nccl",
                    help="nccl: one GPU per rank; gloo: all ranks on GPU 0")
    ap.add_argument("--epochs", type=int, default=300)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    if "RANK" not in os.environ:          # the launcher: start one fresh process per rank, touch no GPU here
        codes = parallel.launch_ranks([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], a.ranks)
        sys.exit(max(abs(c) for c in codes) if any(codes) else 0)
    import torch.distributed as dist
    local = int(os.environ.get("LOCAL_RANK", 0))
    torch.cuda.set_device(local if a.backend == "nccl" else 0)
    dist.init_process_group(a.backend)
    try:
        run(epochs=a.epochs, seed=a.seed, device="cuda")
        dist.barrier()
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
