"""Decoupled evaluations on the host: ``JESMOC_MFDGP.get_nextpoint_decoupled`` over stand-in per-black-box values (the models'
arithmetic has no CPU path: the engine choice, the shared raw candidates, the weighting and the pick are what runs here), the
random baseline, ``optimize_acqf_multistart(Xraw=...)`` and ``BlackBoxMFDGPFitter(decoupled_evals=True)``.  No GPU."""
import contextlib
import pickle

import pytest
import torch

from mobocmf_amd.util import synthetic
from tests.helpers import to_t


def _stub_class():
    from mobocmf_amd.acquisition_functions.JESMOC_MFDGP import _JES_MFDGP

    class Stub(_JES_MFDGP):
        """value = height - |X - centre|^2: the maximum ``height`` is attained at ``centre`` (inside the box)."""

        def __init__(self, fidelity, height, centre):
            super().__init__(fidelity, None, None)
            self.height, self.centre, self.calls = height, centre, 0

        def forward(self, X):
            self.calls += 1
            X = X[:, 0, :] if X.dim() > 2 else X
            return self.height - ((X - self.centre) ** 2).sum(-1)
        __call__ = forward

        @contextlib.contextmanager
        def frozen(self):
            yield self

    return Stub


def _acq(heights, costs, centres=None):
    """heights / costs: {fidelity: {name: number}}; names starting with "c" are constraints."""
    from mobocmf_amd.acquisition_functions.JESMOC_MFDGP import JESMOC_MFDGP
    Stub = _stub_class()
    acq = JESMOC_MFDGP.__new__(JESMOC_MFDGP)
    acq.num_fidelities, acq.eval_highest_fidelity = len(heights), False
    acq.standard_bounds = torch.tensor([[0.0], [1.0]], dtype=torch.float64)
    acq.objectives, acq.constraints, acq.costs_blackboxes = {}, {}, {}
    for f, boxes in heights.items():
        acq.objectives[f], acq.constraints[f], acq.costs_blackboxes[f] = {}, {}, {"total": 0.0}
        for k, (name, h) in enumerate(boxes.items()):
            c = 0.2 + 0.1 * k + 0.3 * f if centres is None else centres[f][name]
            (acq.constraints if name.startswith("c") else acq.objectives)[f][name] = Stub(f, h, c)
            acq.costs_blackboxes[f][name] = costs[f][name]
            acq.costs_blackboxes[f]["total"] += costs[f][name]
    return acq


def _gen():
    return torch.Generator().manual_seed(7)


HEIGHTS = {0: {"a": 1.0, "con": 1.5, "b": 2.0}, 1: {"a": 9.0, "con": 12.0, "b": 4.0}}
COSTS = {0: {"a": 1.0, "con": 1.0, "b": 1.0}, 1: {"a": 10.0, "con": 10.0, "b": 10.0}}


def test_the_pick_follows_value_over_cost_and_the_tuple_is_well_formed():
    acq = _acq(HEIGHTS, COSTS)
    assert [(n, c) for n, c, _ in acq._boxes(0)] == [("a", False), ("b", False), ("con", True)]      # objectives, then constraints
    out = {}
    for engine in ("host", "device"):      # CPU bounds: both run the host engine
        acq.search = engine
        x, fidelity, name, is_con = acq.get_nextpoint_decoupled(maxiter=15, generator=_gen())
        assert acq.last_search_engine == {0: "host", 1: "host"}
        assert x.shape == (1,) and isinstance(fidelity, int) and isinstance(name, str) and isinstance(is_con, bool)
        out[engine] = (x, fidelity, name, is_con)
        vals = acq.last_decoupled_values
        assert list(vals) == [(0, "a"), (0, "b"), (0, "con"), (1, "a"), (1, "b"), (1, "con")]
        for (f, n), v in vals.items():      # each search found its own box's maximum
            assert abs(v - HEIGHTS[f][n]) < 1e-3, (f, n, v)
        weighed = {k: v / COSTS[k[0]][k[1]] for k, v in vals.items()}
        assert (fidelity, name) == max(weighed, key=weighed.get) == (0, "b") and is_con is False
        assert abs(float(x[0]) - acq.objectives[0]["b"].centre) < 0.05      # that box's candidate
    assert out["host"][1:] == out["device"][1:] and torch.equal(out["host"][0], out["device"][0])


def test_changing_one_cost_changes_the_winner():
    costs = {f: dict(c) for f, c in COSTS.items()}
    costs[1]["con"] = 4.0      # 12 / 4 = 3 > 2 / 1
    x, fidelity, name, is_con = _acq(HEIGHTS, costs).get_nextpoint_decoupled(maxiter=15, generator=_gen())
    assert (fidelity, name, is_con) == (1, "con", True)
    costs[0]["a"] = 0.25       # 1 / 0.25 = 4 > 3
    acq = _acq(HEIGHTS, costs)
    x, fidelity, name, is_con = acq.get_nextpoint_decoupled(maxiter=15, generator=_gen())
    assert (fidelity, name, is_con) == (0, "a", False)
    assert acq.costs_blackboxes[0]["total"] == 2.25      # the total is not what weighs


def test_ties_go_to_the_earlier_fidelity_and_box():
    heights = {0: {"a": 1.0, "b": 1.0, "c": 1.0}, 1: {"a": 2.0, "b": 2.0, "c": 2.0}}
    costs = {0: {"a": 1.0, "b": 1.0, "c": 1.0}, 1: {"a": 4.0, "b": 4.0, "c": 4.0}}
    same = {f: {n: 0.5 for n in heights[f]} for f in heights}      # equal functions from equal candidates: equal bits
    acq = _acq(heights, costs, centres=same)
    x, fidelity, name, is_con = acq.get_nextpoint_decoupled(maxiter=10, generator=_gen())
    v = acq.last_decoupled_values
    assert v[(0, "a")] == v[(0, "b")] == v[(0, "c")] and v[(1, "a")] == v[(1, "b")] == v[(1, "c")]
    assert (fidelity, name, is_con) == (0, "a", False)
    acq.eval_highest_fidelity = True
    assert acq.get_nextpoint_decoupled(maxiter=10, generator=_gen())[1:] == (1, "a", False)
    assert list(acq.last_decoupled_values) == [(1, "a"), (1, "b"), (1, "c")]


def test_all_boxes_of_a_fidelity_start_from_one_draw():
    from mobocmf_amd.acquisition_functions import JESMOC_MFDGP as mod
    acq = _acq(HEIGHTS, COSTS)
    seen = []
    plain = mod.optimize_acqf_multistart

    def spy(fn, bounds, **kw):
        seen.append(kw["Xraw"].clone())
        return plain(fn, bounds, **kw)

    mod.optimize_acqf_multistart = spy
    try:
        acq.get_nextpoint_decoupled(maxiter=2, generator=_gen())
    finally:
        mod.optimize_acqf_multistart = plain
    g = _gen()
    draws = [torch.rand(200, 1, dtype=torch.float64, generator=g) for _ in range(2)]      # bounds [0, 1]: the draw itself
    assert len(seen) == 6 and all(torch.equal(s, draws[k // 3]) for k, s in enumerate(seen))


def test_one_box_returns_the_coupled_point_and_value():
    heights, costs = {0: {"a": 1.0}, 1: {"a": 3.0}}, {0: {"a": 1.0}, 1: {"a": 10.0}}
    acq = _acq(heights, costs)
    x, fidelity, name, is_con = acq.get_nextpoint_decoupled(maxiter=15, generator=_gen())
    cand, fid_c = acq.get_nextpoint_coupled(maxiter=15, generator=_gen())
    assert fidelity == fid_c == 0 and name == "a" and torch.equal(x, cand)
    g = _gen()
    for f in (0, 1):      # the coupled searches from the same generator state, fidelity by fidelity
        c, v = acq._optimize(f, maxiter=15, generator=g)
        assert float(v) == acq.last_decoupled_values[(f, "a")]


def test_raw_candidates_given_are_the_draw_not_made():
    from mobocmf_amd.acquisition_functions.JESMOC_MFDGP import optimize_acqf_multistart
    bounds = torch.tensor([[0.0, -1.0], [2.0, 1.0]], dtype=torch.float64)
    fn = lambda X: -((X - 0.4) ** 2).sum(-1)
    want = optimize_acqf_multistart(fn, bounds, num_restarts=3, raw_samples=50, maxiter=8, generator=_gen())
    Xraw = bounds[0] + (bounds[1] - bounds[0]) * torch.rand(50, 2, dtype=torch.float64, generator=_gen())
    keep = Xraw.clone()
    got = optimize_acqf_multistart(fn, bounds, num_restarts=3, raw_samples=999, maxiter=8, Xraw=Xraw)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(Xraw, keep)


def test_limits_and_pickling(monkeypatch):
    from mobocmf_amd import parallel
    acq = _acq(HEIGHTS, COSTS)
    acq._decoupled_searches = {0: object()}
    state = pickle.loads(pickle.dumps({k: v for k, v in acq.__getstate__().items() if k not in ("objectives", "constraints")}))
    assert "_decoupled_searches" not in state
    acq.search = "nope"
    with pytest.raises(ValueError):
        acq.get_nextpoint_decoupled(maxiter=1)
    acq.search = "host"
    monkeypatch.setattr(parallel, "_no_group", lambda: False)      # as with surrogates sharded over a process group
    with pytest.raises(ValueError, match="one process"):
        acq.get_nextpoint_decoupled(maxiter=1)


def test_group_box_values_sum_to_the_group_value_bitwise():
    from mobocmf_amd.acquisition_functions.JESMOC_MFDGP import JESMOC_MFDGP
    g = torch.Generator().manual_seed(5)
    for K in (1, 2, 5):
        acq = JESMOC_MFDGP.__new__(JESMOC_MFDGP)
        acq.num_pareto_samples = K
        v = 10.0 ** (4.0 * torch.rand(3 * (1 + K), 17, dtype=torch.float64, generator=g) - 2.0)
        rows = torch.stack([acq._group_box_value(v, p) for p in range(3)])
        assert torch.equal(rows.sum(0), acq._group_value(v)) and bool((rows == 0.0).any()) and bool((rows > 0.0).any())


def test_random_choice_draws_a_registered_fidelity_and_box():
    from mobocmf_amd.acquisition_functions.Random_choice import Random_choice
    rc = Random_choice(input_size=3, num_fidelities=2, seed=1)
    with pytest.raises(ValueError):
        rc.get_nextpoint_decoupled()
    boxes = [(0, "a", False), (0, "c", True), (1, "a", False)]
    for f, n, con in boxes:
        rc.add_blackbox(f, n, cost_evaluation=1.0 + 9.0 * f, is_constraint=con)
    seen = set()
    for _ in range(60):
        x, f, n, con = rc.get_nextpoint_decoupled()
        assert x.shape == (3,) and bool((x >= 0).all()) and bool((x <= 1).all())
        seen.add((f, n, con))
    assert seen == set(boxes)      # 3 x (2/3)^60: never a box missed
    assert rc.get_nextpoint_coupled()[1] in (0, 1)      # the coupled baseline as ever


# ------------------------------------------------------------------ the fitter
def _data():
    prob = synthetic.make_problem(d=2, L=2, M=8, N=12, S=3, seed=0)
    x, y, fid = to_t(prob["x"]), to_t(prob["y"])[:, None], to_t(prob["fid"])[:, None]
    extra = torch.rand(3, 2, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    x2 = torch.cat([x[3:9], extra, x[0:1]], 0)      # six rows seen before, three new ones, one seen before
    return (x, y, fid), (x2, y[:10] + 1.0, fid[:10]), extra


def test_unequal_inputs_need_decoupled_evals():
    from mobocmf_amd.util.blackbox_mfdgp_fitter import BlackBoxMFDGPFitter
    (x, y, fid), (x2, y2, fid2), extra = _data()
    fitter = BlackBoxMFDGPFitter(2, 12, device="cpu")
    fitter.initialize_mfdgp(x, y, fid, "f0")
    with pytest.raises(AssertionError, match="decoupled"):
        fitter.initialize_mfdgp(x2, y2, fid2, "f1")
    fitter.initialize_mfdgp(x.clone(), y + 1.0, fid, "c0", is_constraint=True, threshold_constraint=0.5)
    assert fitter.x_train is x and fitter.objs_train.shape == (12, 1) and torch.equal(fitter.cons_train, y + 1.0)      # as ever


def test_decoupled_evals_keeps_the_ordered_union_of_the_inputs():
    from mobocmf_amd.util.blackbox_mfdgp_fitter import BlackBoxMFDGPFitter
    (x, y, fid), (x2, y2, fid2), extra = _data()
    fitter = BlackBoxMFDGPFitter(2, 12, device="cpu", decoupled_evals=True)
    fitter.initialize_mfdgp(x, y, fid, "f0")
    assert torch.equal(fitter.x_train, x)
    fitter.initialize_mfdgp(x2, y2, fid2, "f1")
    assert torch.equal(fitter.x_train, torch.cat([x, extra], 0))
    fid3 = (torch.arange(8, dtype=torch.float64) % 2)[:, None]      # (a surrogate needs rows of every fidelity)
    fitter.initialize_mfdgp(torch.cat([extra[1:], x[4:10]], 0), y[:8], fid3, "c0", is_constraint=True,
                            threshold_constraint=0.5)
    assert torch.equal(fitter.x_train, torch.cat([x, extra], 0))      # nothing new, no duplicates
    assert fitter.objs_train is None and fitter.cons_train is None
    assert (fitter.num_obj, fitter.num_con) == (2, 1) and fitter.thresholds_cons.tolist() == [0.5]
    sizes = [h.num_data for _, _, h in fitter._handlers()]
    assert sizes == [12, 10, 8] and [h.train_dataset.tensors[0].shape[0] for _, _, h in fitter._handlers()] == sizes
    fitter.set_pareto_solution(x[:4], torch.zeros(4, 2, dtype=torch.float64))
    assert fitter.pareto_set.shape == (4, 2) and fitter.pareto_front.shape == (4, 2)
    copy = fitter.copy_uncond()      # (the conditioned iterations themselves need the GPU: tests/test_hip_decoupled_search.py)
    assert torch.equal(copy.x_train, fitter.x_train) and copy.objs_train is None
