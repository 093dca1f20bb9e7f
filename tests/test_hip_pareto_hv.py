"""mobocmf_pareto_mask / mobocmf_hypervolume on the MI355X: the mask against the reference's MOOP (golden file) and this build's
MOOP.compute_pareto_front (ties, duplicates, feasibility, NaN), the feasibility rule against torch's normal cdf, the
hypervolume against the numpy oracle of test_pareto_hv_cpu and its invariances, BlackBoxMFDGPFitter.recommend against a host
recomputation (one process, and the black-boxes sharded over two spawned processes), and one scored BO iteration of
examples/bo_loop_hv_toy2d.py."""
import ctypes
import os
import sys
import traceback

import numpy as np
import pytest
import torch

from mobocmf_amd import _lib
from mobocmf_amd.util.moop import MOOP
from tests.test_pareto_hv_cpu import hv_oracle

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_moop.npz")
EXAMPLES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples")


def _mask(pts, **kw):
    from mobocmf_amd import functional as F
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(pts, dtype=np.float64).T)).cuda()
    m, c = F.pareto_mask(t, **kw)
    return m.cpu().numpy(), c.cpu().numpy()


def _hv(pts, ref):
    from mobocmf_amd import functional as F
    return F.hypervolume(torch.from_numpy(np.ascontiguousarray(pts, dtype=np.float64)).cuda(), ref)


# ------------------------------------------------------------------ mask
def test_mask_equals_reference_moop_golden():
    G = np.load(GOLDEN)
    for c in range(6):
        m, cnt = _mask(G[f"front_pts_{c}"])
        assert np.array_equal(m, G[f"front_mask_{c}"]), c
        assert cnt[1] == m.sum() and cnt[0] == m.size and cnt[2] == 0


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6, 9, 16])
def test_mask_equals_moop_on_integer_rows(k):
    rng = np.random.default_rng(k)
    sizes = [0, 1, 2, 63, 64, 65, 1000, 5000] + ([200_000] if k in (2, 3) else [])
    for n in sizes:
        pts = rng.integers(0, 6 if k > 3 else 40, size=(n, k)).astype(np.float64)
        if n > 4:
            pts[n // 2] = pts[1]                    # an exact duplicate after its first copy
        m, cnt = _mask(pts)
        ref = MOOP.compute_pareto_front(pts)
        assert np.array_equal(m, ref), (k, n)
        assert cnt.tolist() == [n, int(ref.sum()), 0]


def test_mask_with_random_feasibility_and_nan_rows():
    rng = np.random.default_rng(3)
    n, k = 20000, 3
    pts = rng.integers(0, 30, size=(n, k)).astype(np.float64)
    keep = rng.uniform(size=n) < 0.4
    # a feasibility rule that keeps exactly `keep`: one constraint, m = +-1, v = 1e-4
    cm = torch.from_numpy(np.where(keep, 1.0, -1.0)[None, :]).cuda()
    cv = torch.full((1, n), 1e-4, dtype=torch.float64, device="cuda")
    m, cnt = _mask(pts, con_mean=cm, con_var=cv)
    ref = np.zeros(n, dtype=bool)
    ref[np.flatnonzero(keep)[MOOP.compute_pareto_front(pts[keep])]] = True
    assert np.array_equal(m, ref) and cnt.tolist() == [int(keep.sum()), int(ref.sum()), 0]
    # NaN objectives: never kept, never dominating; counted
    bad = rng.uniform(size=n) < 0.05
    pts2 = pts.copy()
    pts2[bad, rng.integers(0, k, size=int(bad.sum()))] = np.nan
    m, cnt = _mask(pts2)
    ref = np.zeros(n, dtype=bool)
    ref[np.flatnonzero(~bad)[MOOP.compute_pareto_front(pts2[~bad])]] = True
    assert np.array_equal(m, ref) and cnt.tolist() == [n, int(ref.sum()), int(bad.sum())]


def test_feasibility_rule_matches_torch_cdf():
    rng = np.random.default_rng(4)
    n, K, p_min = 50000, 3, 0.999
    m = rng.normal(0, 3, size=(K, n))
    v = rng.uniform(0.01, 2.0, size=(K, n))
    noise = np.array([0.005, 0.0, 0.02])
    special = rng.integers(0, n, size=60)              # v - noise < 0 and == 0, with m > 0, < 0, == 0
    v[0, special[:20]] = noise[0] / 2
    v[0, special[20:40]] = noise[0]
    m[0, special[20:27]] = 0.0
    m[0, special[27:34]] = 1.0
    m[0, special[34:40]] = -1.0
    z = torch.from_numpy(m) / torch.sqrt(torch.from_numpy(v) - torch.from_numpy(noise)[:, None])
    p = torch.distributions.Normal(0.0, 1.0, validate_args=False).cdf(z).numpy()
    near = np.abs(p - p_min) < 1e-12
    m[near] = 50.0                                      # keep every value clear of the threshold
    z = torch.from_numpy(m) / torch.sqrt(torch.from_numpy(v) - torch.from_numpy(noise)[:, None])
    feas = np.all(torch.distributions.Normal(0.0, 1.0, validate_args=False).cdf(z).numpy() > p_min, axis=0)
    obj = rng.uniform(size=(n, 2))
    mk, cnt = _mask(obj, con_mean=torch.from_numpy(m).cuda(), con_var=torch.from_numpy(v).cuda(),
                    noise=torch.from_numpy(noise).cuda(), p_min=p_min)
    assert cnt[0] == feas.sum()
    ref = np.zeros(n, dtype=bool)
    ref[np.flatnonzero(feas)[MOOP.compute_pareto_front(obj[feas])]] = True
    assert np.array_equal(mk, ref)


# ------------------------------------------------------------------ hypervolume
def _front(rng, P, k, kind):
    if kind == "simplex":
        x = np.abs(rng.normal(size=(P, k)))
        return x / np.linalg.norm(x, axis=1, keepdims=True)
    return rng.uniform(size=(P, k))


@pytest.mark.parametrize("k,P,kind", [(1, 50, "uniform"), (2, 8, "uniform"), (2, 3000, "simplex"), (3, 9, "simplex"),
                                      (3, 500, "uniform"), (3, 2000, "simplex"), (4, 10, "uniform"), (4, 120, "simplex"),
                                      (4, 300, "simplex"), (5, 8, "simplex"), (5, 40, "simplex")])
def test_hypervolume_matches_oracle(k, P, kind):
    rng = np.random.default_rng(100 * k + P)
    pts = _front(rng, P, k, kind)
    ref = np.full(k, 1.05)
    hv = _hv(pts, ref)
    exact = hv_oracle(pts, ref)
    assert hv == pytest.approx(exact, rel=1e-11, abs=0.0)


def test_hypervolume_invariances_and_edges():
    rng = np.random.default_rng(9)
    pts = _front(rng, 200, 3, "simplex")
    ref = np.array([1.1, 1.2, 1.05])
    hv = _hv(pts, ref)
    assert _hv(pts, ref) == hv                                        # bitwise, call to call
    perm, cols = rng.permutation(200), np.array([2, 0, 1])
    assert _hv(pts[perm][:, cols], ref[cols]) == pytest.approx(hv, rel=1e-12)
    dominated = pts[:50] + rng.uniform(0.0, 0.05, size=(50, 3))
    more = np.concatenate([pts, dominated, pts[:30], np.full((5, 3), 2.0)])  # dominated, duplicates, outside ref
    assert _hv(more[rng.permutation(more.shape[0])], ref) == pytest.approx(hv, rel=1e-12)
    assert _hv(2.0 * pts, 2.0 * ref) == pytest.approx(8.0 * hv, rel=1e-13)
    assert _hv(np.zeros((0, 3)), ref) == 0.0
    assert _hv(pts + 5.0, ref) == 0.0
    assert _hv(np.array([[0.5, 1.2, 0.1]]), ref) == 0.0               # on the boundary of ref: no volume


def test_hypervolume_bounds_and_nan_refused():
    from mobocmf_amd import functional as F
    lib = _lib.require_device()
    nb = ctypes.c_size_t()
    for k, P in [(3, 65536), (4, 1024), (5, 256), (1, 65536)]:
        assert lib.mobocmf_hypervolume_workspace_bytes(k, P, ctypes.byref(nb)) == _lib.OK
    for k, P in [(3, 65537), (4, 1025), (5, 257), (6, 2), (0, 2)]:
        assert lib.mobocmf_hypervolume_workspace_bytes(k, P, ctypes.byref(nb)) == _lib.BAD_ARG
        out = ctypes.c_double()
        assert lib.mobocmf_hypervolume(k, P, None, max(k, 1), None, ctypes.byref(out), None, 0, None) == _lib.BAD_ARG
    with pytest.raises(_lib.MobocmfError):
        _hv(np.random.default_rng(0).uniform(size=(1025, 4)), np.ones(4))
    pts = np.random.default_rng(1).uniform(size=(20, 3))
    pts[7, 1] = np.nan
    with pytest.raises(_lib.MobocmfError):
        _hv(pts, np.ones(3))
    with pytest.raises(_lib.MobocmfError):
        F.hypervolume(torch.zeros(3, 2, dtype=torch.float64, device="cuda"), [1.0, float("nan")])


def test_hv_class_is_pymoo_call_form():
    from mobocmf_amd.util.hypervolume import HV
    rng = np.random.default_rng(2)
    pts = rng.uniform(size=(3000, 2))
    ind = HV(ref_point=np.array([1000.0, 1000.0]))
    assert ind(pts) == pytest.approx(hv_oracle(pts, [1000.0, 1000.0]), rel=1e-12)
    assert ind(torch.from_numpy(pts)) == ind(pts)
    assert ind(np.array([1.0, 2.0])) == pytest.approx(999.0 * 998.0, rel=1e-15)
    assert ind(np.zeros((0, 2))) == 0.0


# ------------------------------------------------------------------ recommend
NAMES = [("obj1", False), ("obj2", False), ("con1", True), ("con2", True)]


def _toy_fitter(seed=0, epochs=40):
    from mobocmf_amd.models.mfdgp import TL
    from mobocmf_amd.util.blackbox_mfdgp_fitter import BlackBoxMFDGPFitter
    torch.manual_seed(seed)
    rng = np.random.default_rng(seed)
    x = rng.uniform(size=(24, 2))
    fid = np.concatenate([np.zeros(16), np.ones(8)])
    fs = {"obj1": lambda x: np.sin(3 * x[:, 0]) + x[:, 1] ** 2, "obj2": lambda x: np.cos(2 * x[:, 0] + 1) * (1 - x[:, 1]),
          "con1": lambda x: 0.9 - x[:, 0] * x[:, 1] - 0.5 * x[:, 0], "con2": lambda x: 0.8 - (x[:, 0] - 0.3) ** 2 - x[:, 1]}
    fitter = BlackBoxMFDGPFitter(2, x.shape[0], num_epochs_1=epochs, num_epochs_2=epochs, type_lengthscale=TL.MEDIAN,
                                 device="cuda")
    fitter.verbose = False
    for name, is_con in NAMES:
        y = fs[name](x) * np.where(fid == 0, 0.9, 1.0)
        fitter.initialize_mfdgp(torch.from_numpy(x), torch.from_numpy(y)[:, None], torch.from_numpy(fid)[:, None], name,
                                is_constraint=is_con)
    fitter.train_mfdgps()
    return fitter


def _host_recommend(fitter, grid):
    x = torch.from_numpy(grid).cuda()
    top = fitter.num_fidelities - 1
    objs, feas = [], np.ones(grid.shape[0], dtype=bool)
    with torch.no_grad():
        for name, is_con in NAMES:
            mf = (fitter.mfdgp_handlers_cons if is_con else fitter.mfdgp_handlers_objs)[name].mfdgp
            m, v = mf.predict_for_acquisition(x, top)
            if is_con:
                v = v - getattr(mf, "hidden_layer_likelihood_%d" % top).noise
                feas &= (torch.distributions.Normal(0.0, 1.0, validate_args=False).cdf(m / torch.sqrt(v)) > 0.999).cpu().numpy()
            else:
                objs.append(m.cpu().numpy())
    objs = np.stack(objs, 1)
    keep = np.flatnonzero(feas)[MOOP.compute_pareto_front(objs[feas])]
    return grid[keep], objs[keep]


def _grid():
    return np.random.default_rng(77).uniform(size=(2000, 2))


def test_recommend_equals_host_recomputation():
    fitter = _toy_fitter()
    grid = _grid()
    ps, pf, info = fitter.recommend(grid)
    hs, hf = _host_recommend(fitter, grid)
    assert ps.shape[0] > 0 and info["num_front"] == ps.shape[0] and info["num_nan"] == 0
    assert np.array_equal(ps, hs) and np.array_equal(pf, hf)
    ref = pf.max(0) + 0.5
    from mobocmf_amd.util.hypervolume import HV
    assert HV(ref_point=ref)(pf) == pytest.approx(hv_oracle(hf, ref), rel=1e-11)


def _sharded_worker(rank, world, port, q):
    try:
        import copy

        import torch.distributed as dist
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        fitter = _toy_fitter()                      # every rank trains all four; each then recommends from its shard
        grid = _grid()
        sub = copy.copy(fitter)
        sub.mfdgp_handlers_objs, sub.mfdgp_handlers_cons = {}, {}
        for tag, i, h in fitter._handlers():
            name = [n for n, hh in list(fitter.mfdgp_handlers_objs.items()) + list(fitter.mfdgp_handlers_cons.items())
                    if hh is h][0]
            if NAMES.index((name, tag == "CON")) % world == rank:
                h.global_index = i
                (sub.mfdgp_handlers_cons if tag == "CON" else sub.mfdgp_handlers_objs)[name] = h
        ps, pf, _ = sub.recommend(grid)
        dist.destroy_process_group()
        full = _host_recommend(fitter, grid)
        q.put((rank, "ok", ps, pf, full[0], full[1]))
    except BaseException:
        q.put((rank, "crashed", traceback.format_exc()))


def test_recommend_sharded_over_two_processes():
    from tests.test_hip_pareto_sharded import _spawn
    from tests.test_parallel_pareto_gloo import _free_port
    res = _spawn(_sharded_worker, (2, _free_port()), 2)
    for r in res:
        _, _, ps, pf, hs, hf = r
        assert ps.shape[0] > 0
        assert np.array_equal(ps, hs) and np.array_equal(pf, hf)
    assert np.array_equal(res[0][2], res[1][2]) and np.array_equal(res[0][3], res[1][3])


# ------------------------------------------------------------------ the scored BO loop
@pytest.mark.parametrize("acq", ["jes", "random"])
def test_bo_loop_hv_one_iteration(acq, tmp_path):
    sys.path.insert(0, EXAMPLES)
    try:
        from bo_loop_hv_toy2d import loop_hv
    finally:
        sys.path.remove(EXAMPLES)
    kw = dict(cond_iters=30, acq_iters=8, grid=40) if acq == "jes" else {}
    rows = loop_hv(iters=1, acq=acq, seed=0, out_dir=str(tmp_path), epochs=60, verbose=False, **kw)
    lines = (tmp_path / "hypervolumes.txt").read_text().strip().splitlines()
    assert len(lines) == 1 and len(rows) == 1
    vals = [float(v) for v in lines[0].split()]
    assert len(vals) == 6
    hv_iter, optimal_hv, feasible, n_inf, n_fini, n_ini = vals
    assert 0.0 <= hv_iter <= optimal_hv * (1 + 1e-9) and optimal_hv > 0
    assert feasible in (0.0, 1.0) and n_inf == n_ini - n_fini and n_fini >= 0
