"""Pareto sampling with the black-boxes sharded over two processes on one card (gloo: RCCL refuses two ranks on one
device), models on the GPU so that MOOP takes the batched kernel path: the same solution on both ranks as in one process
holding everything; one sharded BO iteration of examples/bo_iteration_toy2d_sharded.py end to end; and a one-rank RCCL
group against no group.  The test process itself never touches the GPU: every GPU process is a fresh spawned child, at most
two at a time."""
import os
import sys
import traceback

import numpy as np
import pytest
import torch.multiprocessing as mp

from tests.test_parallel_pareto_gloo import _free_port, check_solution, layout, pareto_setup, run_ranks, solution

pytestmark = pytest.mark.gpu
EXAMPLES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples")


def _spawn(target, args, n, timeout=600):
    """n spawned children of ``target(rank, *args, q)``; results in rank order; no child outlives the call."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=target, args=(r,) + tuple(args) + (q,)) for r in range(n)]
    try:
        for p in procs:
            p.start()
        res = sorted((q.get(timeout=timeout) for _ in range(n)), key=lambda r: r[0])
        for p in procs:
            p.join(timeout=120)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
                p.join(timeout=10)
    for r in res:
        assert r[1] != "crashed", r[2]
    return res


def _single_worker(rank, n_obj, q):
    try:
        from mobocmf_amd.util.moop import MOOP
        fitter = pareto_setup([n for n, _, _ in layout(n_obj)], "cuda", n_obj=n_obj)
        out = solution(fitter)
        batched = MOOP(fitter.samples_objs, fitter.samples_cons, 2)._batched_device() is not None
        q.put((rank, "ok", batched) + out)
    except BaseException:
        q.put((rank, "crashed", traceback.format_exc()))


@pytest.mark.parametrize("n_obj", [2, 3])
def test_sharded_pareto_solution_on_the_gpu_equals_single_process(n_obj):
    res = run_ranks("three" if n_obj == 3 else "two", device="cuda")
    (_, _, batched, *ref), = _spawn(_single_worker, (n_obj,), 1)
    assert batched
    for r in res:
        assert r[1] == "ok"
        ps, pf, objs, cons = r[3:]
        assert np.array_equal(ps, ref[0]) and np.array_equal(pf, ref[1])
        check_solution(ps, pf, objs, cons)
        assert np.all(cons >= -0.1 - 1e-6)


def _example_worker(rank, world, port, q):
    try:
        import torch
        import torch.distributed as dist
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        sys.path.insert(0, EXAMPLES)
        from bo_iteration_toy2d_sharded import run
        fitter, acq, cand, fidelity = run(epochs=60, cond_iters=30, acq_iters=8, grid=40, seed=0, verbose=False)
        ps, pf = fitter.pareto_set.cpu().numpy(), fitter.pareto_front.cpu().numpy()
        objs = np.stack([s(ps) for s in fitter.samples_objs], 1)
        cons = np.stack([s(ps) for s in fitter.samples_cons], 1)
        costs = [acq.costs_blackboxes[f]["total"] for f in range(2)]
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, "ok", cand.cpu().numpy(), int(fidelity), ps, pf, objs, cons, costs))
    except BaseException:
        q.put((rank, "crashed", traceback.format_exc()))


def test_sharded_bo_iteration_end_to_end():
    res = _spawn(_example_worker, (2, _free_port()), 2, timeout=900)
    (_, _, c0, f0, ps0, pf0, *_), (_, _, c1, f1, ps1, pf1, *_) = res
    assert np.array_equal(c0, c1) and f0 == f1                             # the same decision on both ranks
    assert np.array_equal(ps0, ps1) and np.array_equal(pf0, pf1)
    assert c0.shape == (2,) and 0.0 <= c0.min() and c0.max() <= 1.0 and f0 in (0, 1)
    for _, _, _, _, ps, pf, objs, cons, costs in res:
        assert pf.shape == (ps.shape[0], 2) and objs.shape == pf.shape and cons.shape == (ps.shape[0], 1)
        assert np.abs(objs - pf).max() <= 1e-9                            # ALL objective samples at the stored set
        assert np.all(cons >= -1e-6)
        for p in pf:
            assert np.all(pf[np.all(pf <= p, axis=1)] == p)                # non-dominated
        assert costs == [3.0, 30.0]                                        # every black-box's cost, on every rank


def _nccl_worker(rank, port, q):
    try:
        import torch
        import torch.distributed as dist
        torch.cuda.set_device(0)
        fitter = pareto_setup([n for n, _, _ in layout(2)], "cuda")
        alone = solution(fitter)
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("nccl", rank=0, world_size=1)
        grouped = solution(pareto_setup([n for n, _, _ in layout(2)], "cuda"))
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, "ok", alone, grouped))
    except BaseException:
        q.put((rank, "crashed", traceback.format_exc()))


def test_one_rank_rccl_group_gives_the_same_solution_as_no_group():
    (_, _, alone, grouped), = _spawn(_nccl_worker, (_free_port(),), 1)
    for a, b in zip(alone, grouped):
        assert np.array_equal(a, b)
