"""Pareto sampling with the black-boxes sharded over ranks (world size 2, gloo, spawned children, models on the host): the
seeded joint procedure of ``BlackBoxMFDGPFitter.sample_and_store_pareto_solution`` must store bitwise the same Pareto set
and front on every rank, equal to one process holding every black-box, and every rank must hold every black-box's sample.
The layout is the ragged one round-robin sharding makes: 2 objectives + 1 constraint on 2 ranks, rank 1 holds no
constraint."""
import os
import socket
import traceback

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from mobocmf_amd.util import synthetic

N, D, SEED = 12, 2, 7


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def layout(n_obj):
    """(name, is_constraint, global index) of every black-box of the problem."""
    return [("obj%d" % k, False, k) for k in range(n_obj)] + [("con0", True, 0)]


def pareto_setup(names_mine, device="cpu", n_obj=2, threshold=0.1, duplicate_index=False):
    """A fitter holding the black-boxes ``names_mine`` of ``layout(n_obj)`` (models with fixed parameters, no training),
    with the training inputs and the global threshold vector set."""
    from mobocmf_amd.mlls import VariationalELBOMF
    from mobocmf_amd.util.blackbox_mfdgp_fitter import BlackBoxMFDGPFitter, MFDGPHandler
    fitter = BlackBoxMFDGPFitter(2, N, opt_grid_size=20, pareto_set_size=8, device=device)
    fitter.verbose = False
    x_train = None
    for o, (name, is_con, gi) in enumerate(layout(n_obj)):
        prob = synthetic.make_problem(d=D, L=2, M=8, N=N, S=1, output=o, seed=o)
        x_train = torch.as_tensor(prob["x"], dtype=torch.float64)
        if name not in names_mine:
            continue
        model = synthetic.model_from_problem(prob, num_samples_for_training=1, device=device)
        h = MFDGPHandler.__new__(MFDGPHandler)
        h.mfdgp, h.num_data, h.num_fidelities, h.batch_size = model, N, 2, N
        h.global_index = 0 if (duplicate_index and not is_con) else gi
        h.elbo = VariationalELBOMF(model, N, 2)
        h.iter_train_loader = None
        (fitter.mfdgp_handlers_cons if is_con else fitter.mfdgp_handlers_objs)[name] = h
    fitter.num_obj, fitter.num_con = len(fitter.mfdgp_handlers_objs), len(fitter.mfdgp_handlers_cons)
    fitter.thresholds_cons = torch.tensor([threshold] * fitter.num_con, dtype=torch.float64)
    fitter.set_global_constraint_thresholds([threshold])
    fitter.x_train = x_train.to(device)
    return fitter


def solution(fitter, seed=SEED):
    fitter.sample_and_store_pareto_solution(seed=seed, nFeatures=64)
    ps, pf = fitter.pareto_set.cpu().numpy(), fitter.pareto_front.cpu().numpy()
    objs = np.stack([s(ps) for s in fitter.samples_objs], 1)
    cons = np.stack([s(ps) for s in fitter.samples_cons], 1)
    return ps, pf, objs, cons


def _worker(rank, world, port, case, q, device="cpu", max_tries=None):
    try:
        import torch.distributed as dist
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from mobocmf_amd import parallel
        from mobocmf_amd.util.blackbox_mfdgp_fitter import MFDGPHandler
        if max_tries is not None:
            MFDGPHandler.MAX_TRIES_FOR_FEASIBLE_GRID = max_tries
        n_obj = 3 if case == "three" else 2
        mine, _ = parallel.shard_blackboxes([n for n, _, _ in layout(n_obj)])
        fitter = pareto_setup(mine, device, n_obj=n_obj, threshold=-1e6 if case == "infeasible" else 0.1,
                              duplicate_index=case == "duplicate")
        try:
            out = ("ok", mine) + solution(fitter)
        except Exception as e:
            out = ("raised", mine, type(e).__name__, str(e))
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank,) + out)
    except BaseException:
        q.put((rank, "crashed", traceback.format_exc()))


def run_ranks(case, world=2, **kw):
    """Spawns the ranks, returns their results in rank order; no child outlives the call."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, case, q), kwargs=kw) for r in range(world)]
    try:
        for p in procs:
            p.start()
        res = sorted((q.get(timeout=300) for _ in range(world)), key=lambda r: r[0])
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
                p.join(timeout=10)
    for r in res:
        assert r[1] != "crashed", r[2]
    return res


def check_solution(ps, pf, objs, cons):
    assert ps.ndim == 2 and ps.shape[1] == D and 1 <= ps.shape[0] <= 8 and pf.shape[0] == ps.shape[0]
    assert np.allclose(objs, pf, rtol=0, atol=1e-9)            # every rank's samples reproduce the front at the set
    for p in pf:          # non-dominated (the summary may pick one point twice: the best of two objectives)
        assert np.all(pf[np.all(pf <= p, axis=1)] == p)


@pytest.mark.parametrize("case", ["two", "three"])
def test_sharded_pareto_solution_equals_single_process(case):
    n_obj = 3 if case == "three" else 2
    ref = solution(pareto_setup([n for n, _, _ in layout(n_obj)], n_obj=n_obj))
    res = run_ranks(case)
    if n_obj == 2:
        assert res[0][2] == ["obj0", "con0"] and res[1][2] == ["obj1"]       # ragged: rank 1 holds no constraint
    else:
        assert res[0][2] == ["obj0", "obj2"] and res[1][2] == ["obj1", "con0"]
    for r in res:
        assert r[1] == "ok"
        ps, pf, objs, cons = r[3:]
        assert np.array_equal(ps, ref[0]) and np.array_equal(pf, ref[1])      # bitwise, = one process with everything
        assert pf.shape[1] == n_obj and cons.shape[1] == 1
        check_solution(ps, pf, objs, cons)
        assert np.all(cons >= -0.1 - 1e-6)
        assert np.array_equal(objs, ref[2]) and np.array_equal(cons, ref[3])


def test_all_tries_infeasible_every_rank_takes_the_same_fallback(monkeypatch):
    from mobocmf_amd.util.blackbox_mfdgp_fitter import MFDGPHandler
    monkeypatch.setattr(MFDGPHandler, "MAX_TRIES_FOR_FEASIBLE_GRID", 2)
    ref = solution(pareto_setup(["obj0", "obj1", "con0"], threshold=-1e6))
    res = run_ranks("infeasible", max_tries=2)
    for r in res:
        assert r[1] == "ok"
        assert np.array_equal(r[3], ref[0]) and np.array_equal(r[4], ref[1])
        assert np.all(r[6] < 1e6)                                # the least infeasible points: still infeasible
    assert np.array_equal(res[0][3], res[1][3])


def test_duplicated_global_index_raises_on_every_rank():
    res = run_ranks("duplicate")
    for r in res:
        assert r[1] == "raised" and r[3] == "ValueError" and "permutation" in r[4], r
    assert res[0][4] == res[1][4]
