"""JES per black-box on the host: the restatement of mobocmf_jes_mc_box_forward (tests/jes_box_reference.py) against
torch.autograd on term_b and, bit for bit, against the coupled restatement (tests/jes_mc_reference.py); the entry point's host
checks.  No GPU."""
import ctypes

import pytest
import torch

from tests import jes_box_reference as RB
from tests import jes_mc_reference as R

SHAPES = [(1, 1, 1, 1), (3, 1, 6, 4), (2, 4, 5, 4), (3, 2, 67, 1), (32, 1, 3, 2), (2, 8, 200, 5)]


def _bits(t):
    return t.detach().contiguous().view(torch.int64)


@pytest.mark.parametrize("n_boxes,K,T,S", SHAPES)
def test_all_box_rows_sum_to_the_coupled_value_bitwise(n_boxes, K, T, S):
    """P1 on the host: the rows accumulated in the order of p from 0.0 ARE jes_mc_group_forward's acq."""
    kinds = set()
    for flip in range(4):
        mom, noise = R.mc_inputs(n_boxes, K, T, S, seed=10 * T + S + K, flip=flip)
        rows, scale = RB.jes_mc_box_all(mom, noise, K, T, S)
        acq, _, scale_c = R.jes_mc_group_forward(mom, noise, K, T, S, want_seeds=False)
        total, sc = torch.zeros(T, dtype=torch.float64), torch.zeros(T, dtype=torch.float64)
        for p in range(n_boxes):
            total = total + rows[p]
            sc = sc + scale[p]
        assert rows.shape == (n_boxes, T) and torch.equal(_bits(total), _bits(acq))
        assert float(((sc - scale_c) / scale_c).abs().max()) <= 1e-15      # (a bound's scale: summed in another order)
        count = R.passing(mom, noise, K, T, S).sum(1)
        kinds |= {"none" if c == 0 else "all" if c == K else "some" for c in count.reshape(-1).tolist()}
        assert bool((rows[count == 0] == 0.0).all()) and bool((rows[count > 0] > 0.0).all())
    assert kinds == ({"none", "some", "all"} if K >= 2 else {"none", "all"})


@pytest.mark.parametrize("n_boxes,K,T,S", SHAPES)
def test_selected_box_seeds_are_the_autograd_gradient_of_term_b(n_boxes, K, T, S):
    for flip in range(4):
        mom, noise = R.mc_inputs(n_boxes, K, T, S, seed=10 * T + S + K, flip=flip)
        rows, _ = RB.jes_mc_box_all(mom, noise, K, T, S)
        _, seeds_c, _ = R.jes_mc_group_forward(mom, noise, K, T, S)
        for name, box in RB.box_patterns(n_boxes, T).items():
            assert int(box.min()) == 0 and int(box.max()) == min(n_boxes, T) - 1, name
            acq, seeds, _ = RB.jes_mc_box_selected(mom, noise, K, T, S, box)
            assert torch.equal(_bits(acq), _bits(rows[box.long(), torch.arange(T)]))      # P2, values
            m = mom.clone().requires_grad_(True)
            val = RB.jes_box_value(m, noise, K, T, S, box)
            assert float((val.detach() - acq).abs().max()) <= 1e-14 * float(acq.abs().max().clamp_min(1.0))
            val.sum().backward()
            assert float((seeds - m.grad).abs().max()) <= 1e-13 * float(m.grad.abs().max().clamp_min(1e-300))
            own = (torch.arange(mom.shape[0])[:, None] // (1 + K) == box[None, :].long())
            own = own[:, None, :, None].expand(mom.shape[0], 2, T, S).reshape(mom.shape)
            assert torch.equal(_bits(seeds[own]), _bits(seeds_c[own]))                     # P2, the box's own models
            assert bool((_bits(seeds[~own]) == 0).all())                                   # every other seed: +0.0
            assert bool((m.grad[~own] == 0.0).all())


def test_one_box_is_the_coupled_restatement_and_a_bad_word_gives_nan():
    K, T, S = 3, 9, 2
    mom, noise = R.mc_inputs(1, K, T, S, seed=4, flip=1)
    acq, seeds, scale = RB.jes_mc_box_selected(mom, noise, K, T, S, torch.zeros(T, dtype=torch.int32))
    acq_c, seeds_c, scale_c = R.jes_mc_group_forward(mom, noise, K, T, S)
    assert torch.equal(_bits(acq), _bits(acq_c)) and torch.equal(_bits(seeds), _bits(seeds_c))      # P3
    mom, noise = R.mc_inputs(2, K, T, S, seed=5, flip=0)
    box = torch.tensor([0, 1, 2, -1, 1, 0, 7, 1, 0], dtype=torch.int32)
    acq, seeds, _ = RB.jes_mc_box_selected(mom, noise, K, T, S, box)
    bad = (box < 0) | (box >= 2)
    assert torch.equal(torch.isnan(acq), bad)
    cols = bad[:, None].expand(T, S).reshape(T * S)
    assert bool((seeds[:, :, cols] == 0.0).all()) and bool((seeds[:, :, ~cols] != 0.0).any())


def test_entry_point_refuses_bad_arguments_without_a_device():
    from mobocmf_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)      # never dereferenced: every call below is refused before any device call

    def box(moments=p, noise=p, n_boxes=2, K=2, T=3, S=2, words=p, acq=p, acq_ld=0, want_seeds=1, seeds=p, track=1, x=p, d=2,
            best_v=p, best_x=p):
        return lib.mobocmf_jes_mc_box_forward(moments, noise, n_boxes, K, T, S, words, acq, acq_ld, want_seeds, seeds, track, x, d,
                                              best_v, best_x, None)

    for kw in (dict(n_boxes=0), dict(K=0), dict(n_boxes=22), dict(T=0), dict(S=0), dict(moments=None), dict(noise=None),
               dict(acq=None), dict(seeds=None), dict(x=None), dict(best_v=None), dict(best_x=None), dict(d=0), dict(d=33),
               dict(want_seeds=2), dict(track=-1), dict(T=1 << 20, S=1 << 10)):      # the coupled entry point's conditions
        assert box(**kw) == _lib.BAD_ARG, kw
    allbox = dict(words=None, want_seeds=0, track=0, acq_ld=3)
    for kw in (dict(acq_ld=2), dict(acq_ld=0), dict(want_seeds=1), dict(track=1)):      # the all-box mode's own
        assert box(**dict(allbox, **kw)) == _lib.BAD_ARG, kw
