"""What the small-layer natural-gradient launch relies on that needs no GPU: the triangle-only form of B it builds, and the
fitter's argument rule for ``natgrad_one_launch``."""
import pytest
import torch

from tests import natgrad_reference as R
from tests.test_hip_natgrad import _layer_inputs


@pytest.mark.parametrize("M", [8, 16, 17, 32, 33, 70, 128])
def test_triangle_only_B_is_the_restatements_B_bitwise(M):
    """B = I + gamma scale (tril(P) + tril(P, -1)^T) with P = tril(L_S^T tril(g_LS)) -- only the lower triangle of L_S^T g_LS is
    ever formed -- equals I + 2 gamma scale sym(Phi(P)) of the restatement bit for bit: halving and doubling are exact."""
    gamma, scale = 0.7, 3.0
    for z in range(3):
        m, L_S, g_m, g_LS = _layer_inputs(M, 100 * M + z)
        B_ref = R.natgrad_update(m, L_S, g_m, g_LS, gamma, scale)[2]
        P = torch.tril(torch.tril(L_S).T @ torch.tril(g_LS))
        B = torch.eye(M, dtype=torch.float64) + gamma * scale * (P + torch.tril(P, -1).T)
        assert torch.equal(B, B_ref)


def test_natgrad_one_launch_needs_natural_gradients():
    from mobocmf_amd.util.blackbox_mfdgp_fitter import BlackBoxMFDGPFitter
    with pytest.raises(ValueError):
        BlackBoxMFDGPFitter(2, 8, device="cpu", natgrad_one_launch=True)
    with pytest.raises(ValueError):
        BlackBoxMFDGPFitter(2, 8, device="cpu", variational_optimizer="adam", natgrad_one_launch=True)
    assert BlackBoxMFDGPFitter(2, 8, device="cpu", variational_optimizer="natgrad").natgrad_one_launch is False
    assert BlackBoxMFDGPFitter(2, 8, device="cpu", variational_optimizer="natgrad", natgrad_one_launch=True).natgrad_one_launch
