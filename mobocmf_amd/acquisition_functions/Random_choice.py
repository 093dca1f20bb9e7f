"""Random baseline of the BO loop -- mirror of mobocmf/acquisition_functions/Random_choice.py: the same surface, a uniform
point in [0, 1]^d and a fidelity drawn with probability proportional to 1 - (coupled cost of the fidelity) / (total cost).

Difference: ``seed=None`` leaves torch's global generator alone (the reference calls ``torch.manual_seed(None)``, which
raises); any other seed seeds it, as there.
"""
import torch
from torch import Tensor


class Random_choice():

    def __init__(self, input_size=None, num_fidelities: int = 1, seed=None) -> None:
        self.input_size = input_size
        self.num_fidelities = num_fidelities
        self.seed = seed
        if seed is not None:
            torch.manual_seed(seed)
        self.costs_blackboxes = {}
        for n_f in range(num_fidelities):
            self.costs_blackboxes[n_f] = {"total": 0.0}
        self.coupled_costs_fidelities = torch.zeros(self.num_fidelities)
        self.total_cost_fidelities = 0.0

    def add_blackbox(self, fidelity: int, blackbox_name: str, cost_evaluation: float = 1.0, is_constraint: bool = False):
        self.costs_blackboxes[fidelity][blackbox_name] = cost_evaluation
        self.coupled_costs_fidelities[fidelity] += cost_evaluation
        self.total_cost_fidelities += cost_evaluation
        self.__dict__.setdefault("blackboxes", []).append((fidelity, blackbox_name, bool(is_constraint)))

    def get_nextpoint_decoupled(self, iteration=None, verbose=False):
        """The baseline of the decoupled setting: a uniformly chosen registered (fidelity, black-box) and a uniform point.
        Returns (x (d,), fidelity, blackbox_name, is_constraint), as JESMOC_MFDGP.get_nextpoint_decoupled."""
        boxes = self.__dict__.get("blackboxes", [])
        if not boxes:
            raise ValueError("get_nextpoint_decoupled: no black-box registered (add_blackbox)")
        nextpoint = torch.rand(size=(self.input_size,))
        fidelity, name, is_constraint = boxes[int(torch.randint(len(boxes), (1,)).item())]
        if verbose:
            print("Iter:", iteration, " Evaluating", "constraint" if is_constraint else "objective", name, "at fidelity",
                  fidelity, "at", nextpoint.numpy())
        return nextpoint, fidelity, name, is_constraint

    def decoupled_acq(self, X: Tensor, fidelity: int, blackbox_name) -> Tensor:
        return torch.rand(size=(X.shape[0],))

    def coupled_acq(self, X: Tensor, fidelity: int) -> Tensor:
        return torch.rand(size=(X.shape[0],))

    def get_nextpoint_coupled(self, iteration=None, verbose=False):
        fidelities = torch.arange(self.num_fidelities)
        # the probability of choosing a fidelity is one minus its normalised cost
        probs_fidelities = 1.0 - (self.coupled_costs_fidelities / self.total_cost_fidelities)
        nextpoint = torch.rand(size=(self.input_size,))
        fidelity_to_evaluate = fidelities[torch.multinomial(probs_fidelities, 1).item()].item()
        if verbose:
            print("Iter:", iteration, " Evaluating fidelity", fidelity_to_evaluate, "at", nextpoint.numpy())
        return nextpoint, fidelity_to_evaluate
