"""MESMOC_MFGP's search keyword and generator on the CPU: the host engine's bits are unchanged, the keyword is checked when a
search starts, and CPU models keep the host engine whatever the keyword."""
import pytest
import torch

from mobocmf_amd.acquisition_functions.JESMOC_MFDGP import optimize_acqf_multistart
from tests import mes_reference as M

MAXITER = 3


def test_bogus_search_raises_when_a_search_starts():
    acq = M.mes_problem(12, search="bogus")      # (a plain attribute: the constructor takes anything)
    assert acq.search == "bogus"
    with pytest.raises(ValueError, match="search must be"):
        acq.get_nextpoint_coupled(maxiter=1)
    acq.search = "host"
    acq.get_nextpoint_coupled(maxiter=1)


def test_default_search_is_the_direct_host_loop_bit_for_bit():
    acq = M.mes_problem(12)
    assert acq.search == "host"
    torch.manual_seed(11)
    cand, fidelity = acq.get_nextpoint_coupled(maxiter=MAXITER)
    assert acq.last_search_engine == {0: "host", 1: "host"}
    torch.manual_seed(11)
    best = None
    for f in range(acq.num_fidelities):
        c, v = optimize_acqf_multistart(lambda x: acq.coupled_acq(x, fidelity=f), acq.standard_bounds, num_restarts=5,
                                        raw_samples=200, maxiter=MAXITER)
        w = v / acq.costs_blackboxes[f]["total"]
        if best is None or best[0] < w:
            best = (w, c, f)
    assert fidelity == best[2] and torch.equal(cand, best[1][0, :])


def test_generator_makes_two_host_searches_equal():
    acq = M.mes_problem(12)
    out = []
    for _ in range(2):
        torch.manual_seed(len(out))      # (the global state differs: only the generator decides)
        out.append(acq.get_nextpoint_coupled(maxiter=MAXITER, generator=torch.Generator().manual_seed(5)))
    assert out[0][1] == out[1][1] and torch.equal(out[0][0], out[1][0])
    other = acq.get_nextpoint_coupled(maxiter=MAXITER, generator=torch.Generator().manual_seed(6))
    assert not torch.equal(other[0], out[0][0])


def test_cpu_models_keep_the_host_engine_under_search_device():
    acq = M.mes_problem(12, search="device")
    ref = M.mes_problem(12)
    cand, fidelity = acq.get_nextpoint_coupled(maxiter=MAXITER, generator=torch.Generator().manual_seed(5))
    rc, rf = ref.get_nextpoint_coupled(maxiter=MAXITER, generator=torch.Generator().manual_seed(5))
    assert acq.last_search_engine == {0: "host", 1: "host"}
    assert fidelity == rf and torch.equal(cand, rc)
    assert set(acq.last_search_values) == {0, 1}
