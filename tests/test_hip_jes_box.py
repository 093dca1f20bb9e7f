"""JES per black-box on the device (mobocmf_jes_mc_box_forward in csrc/acq_search.hip): the kernel against its float64
restatement (tests/jes_box_reference.py) in both modes, and bit for bit against mobocmf_jes_mc_group_forward on the same inputs
(the properties P1 - P3 of include/mobocmf_hip.h)."""
import pytest
import torch

from tests import acq_search_reference as R1
from tests import jes_box_reference as RB
from tests import jes_mc_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(1, 1, 1, 1), (3, 1, 6, 4), (2, 4, 5, 4), (3, 2, 67, 1), (32, 1, 3, 2), (2, 8, 200, 5)]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int64)


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float64, device=DEV)


# ------------------------------------------------------------------ G1. the kernel against the restatement
@pytest.mark.parametrize("n_boxes,K,T,S", SHAPES)
def test_jes_mc_box_forward_matches_the_reference(n_boxes, K, T, S):
    """Both modes, both box patterns, the four clamp patterns of jes_mc_reference.mc_inputs.  The all-box launch writes a chunk
    of a wider (n_boxes, n) array: what lies outside the chunk's columns is not touched."""
    from mobocmf_amd import functional as F
    for flip in range(4):
        mom, noise = R.mc_inputs(n_boxes, K, T, S, seed=10 * T + S + K, flip=flip)
        rows_ref, scale = RB.jes_mc_box_all(mom, noise, K, T, S)
        md, nd = mom.to(DEV), noise.to(DEV)
        wide = _nan(n_boxes, T + 5)
        F.jes_mc_box_forward(md, nd, K, T, S, wide[:, 2:2 + T])
        torch.cuda.synchronize()
        rows = wide[:, 2:2 + T].cpu()
        assert bool(torch.isnan(wide[:, :2]).all()) and bool(torch.isnan(wide[:, 2 + T:]).all())
        err = (rows - rows_ref).abs()
        print("jes_mc_box_forward all boxes", (n_boxes, K, T, S), "flip", flip, "err / bound", float((err / (1e-14 * (1.0 + scale))).max()))
        assert bool((err <= 1e-14 * (1.0 + scale)).all())
        for name, box in RB.box_patterns(n_boxes, T).items():
            acq_ref, seeds_ref, sc = RB.jes_mc_box_selected(mom, noise, K, T, S, box)
            acq, seeds = _nan(T), torch.full_like(md, float("nan"))
            F.jes_mc_box_forward(md, nd, K, T, S, acq, box_of_point=box.to(DEV), seeds=seeds)
            acq2 = _nan(T)
            F.jes_mc_box_forward(md, nd, K, T, S, acq2, box_of_point=box.to(DEV))      # want_seeds = 0: the same values
            torch.cuda.synchronize()
            err = (acq.cpu() - acq_ref).abs()
            print("  selected", name, "acq err / bound", float((err / (1e-14 * (1.0 + sc))).max()), "seeds rel",
                  float((seeds.cpu() - seeds_ref).abs().max() / seeds_ref.abs().max().clamp_min(1e-300)))
            assert bool((err <= 1e-14 * (1.0 + sc)).all())
            assert float((seeds.cpu() - seeds_ref).abs().max()) <= 1e-12 * float(seeds_ref.abs().max())
            assert torch.equal(_bits(acq), _bits(acq2))


def test_jes_mc_box_forward_tracks_the_best_iterate():
    """Three consecutive calls: the larger value and its row stay (strict), -inf is replaced by any finite value, a NaN value
    (of the point's OWN box) never replaces anything; a NaN in another box's model does not reach the point."""
    from mobocmf_amd import functional as F
    n_boxes, K, T, S, d = 2, 3, 70, 2, 3
    g = torch.Generator().manual_seed(2)
    box = RB.box_patterns(n_boxes, T)["interleaved"]      # test point 0: box 0, test point 1: box 1, ...
    best_v = torch.full((T,), float("-inf"), dtype=torch.float64, device=DEV)
    best_x = torch.zeros(T, d, dtype=torch.float64, device=DEV)
    acq = torch.zeros(T, dtype=torch.float64, device=DEV)
    for call in range(3):
        mom, noise = R.mc_inputs(n_boxes, K, T, S, seed=20 + call, flip=call)
        if call == 0:
            mom[1 + K + 2, 1, S:2 * S] = float("nan")      # test point 1, a conditioned model of box 1: no value
            mom[1 + K + 2, 1, 2 * S:3 * S] = float("nan")  # test point 2 is searched for box 0: box 1's NaN stays out
        if call == 1:
            mom[0, 1, :S] = float("nan")                   # test point 0, the unconditioned model of box 0
        x = torch.rand(T, d, dtype=torch.float64, generator=g)
        prev_v, prev_x = best_v.cpu(), best_x.cpu()
        F.jes_mc_box_forward(mom.to(DEV), noise.to(DEV), K, T, S, acq, box_of_point=box.to(DEV), x=x.to(DEV), best_v=best_v,
                             best_x=best_x)
        torch.cuda.synchronize()
        a, got_v, got_x = acq.cpu(), best_v.cpu(), best_x.cpu()
        acq_ref, _, sc = RB.jes_mc_box_selected(mom, noise, K, T, S, box, want_seeds=False)
        ok = torch.isfinite(acq_ref)
        assert torch.equal(ok, torch.isfinite(a)) and bool(((a - acq_ref).abs()[ok] <= 1e-14 * (1.0 + sc[ok])).all())
        want_v, want_x = R1.track_best(a, x, prev_v, prev_x)
        assert torch.equal(_bits(got_v), _bits(want_v)) and torch.equal(got_x, want_x)
        moved = a > prev_v
        if call == 0:
            assert bool(torch.isnan(a[1])) and float(got_v[1]) == float("-inf") and not bool(got_x[1].any())
            assert bool(torch.isfinite(a[2])) and int(moved.sum()) == T - 1
        if call == 1:
            assert bool(torch.isnan(a[0])) and float(got_v[0]) == float(prev_v[0]) and torch.equal(got_x[0], prev_x[0])
            assert bool(moved[1]) and bool(torch.isfinite(got_v).all())
        if call >= 1:
            assert 0 < int(moved.sum()) < T


# ------------------------------------------------------------------ G2. bit for bit against the coupled kernel
@pytest.mark.parametrize("n_boxes,K,T,S", SHAPES)
def test_all_box_rows_and_selected_box_against_the_coupled_kernel_bitwise(n_boxes, K, T, S):
    from mobocmf_amd import functional as F
    for flip in (0, 3):
        mom, noise = R.mc_inputs(n_boxes, K, T, S, seed=10 * T + S + K, flip=flip)
        md, nd = mom.to(DEV), noise.to(DEV)
        acq_c, seeds_c = _nan(T), torch.full_like(md, float("nan"))
        F.jes_mc_group_forward(md, nd, K, T, S, acq_c, seeds=seeds_c)
        rows, rows2 = _nan(n_boxes, T), _nan(n_boxes, T)
        F.jes_mc_box_forward(md, nd, K, T, S, rows)
        F.jes_mc_box_forward(md, nd, K, T, S, rows2)
        total = torch.zeros(T, dtype=torch.float64, device=DEV)
        for p in range(n_boxes):
            total = total + rows[p]
        assert torch.equal(_bits(total), _bits(acq_c))            # P1
        assert torch.equal(_bits(rows), _bits(rows2))             # two calls: the same bits
        for name, box in RB.box_patterns(n_boxes, T).items():
            acq, seeds = _nan(T), torch.full_like(md, float("nan"))
            F.jes_mc_box_forward(md, nd, K, T, S, acq, box_of_point=box.to(DEV), seeds=seeds)
            acq2, seeds2 = _nan(T), torch.full_like(md, float("nan"))
            F.jes_mc_box_forward(md, nd, K, T, S, acq2, box_of_point=box.to(DEV), seeds=seeds2)
            assert torch.equal(_bits(acq), _bits(rows[box.long().to(DEV), torch.arange(T, device=DEV)]))      # P2
            own = (torch.arange(mom.shape[0])[:, None] // (1 + K) == box[None, :].long())
            own = own[:, None, :, None].expand(mom.shape[0], 2, T, S).reshape(mom.shape)
            s, sc = seeds.cpu(), seeds_c.cpu()
            assert torch.equal(_bits(s[own]), _bits(sc[own])), name
            assert bool((_bits(s[~own]) == 0).all()), name        # every other seed is +0.0: none left as the NaN fill
            assert torch.equal(_bits(acq), _bits(acq2)) and torch.equal(_bits(seeds), _bits(seeds2))


@pytest.mark.parametrize("K,T,S", [(1, 5, 4), (3, 67, 1), (63, 3, 2)])
def test_one_box_with_zero_words_is_the_coupled_entry_point_bitwise(K, T, S):
    """P3, over three consecutive tracked calls."""
    from mobocmf_amd import functional as F
    d = 3
    words = torch.zeros(T, dtype=torch.int32, device=DEV)
    best = {name: (torch.full((T,), float("-inf"), dtype=torch.float64, device=DEV),
                   torch.zeros(T, d, dtype=torch.float64, device=DEV)) for name in ("coupled", "box")}
    g = torch.Generator().manual_seed(K)
    for call in range(3):
        mom, noise = R.mc_inputs(1, K, T, S, seed=40 + call, flip=call)
        md, nd, x = mom.to(DEV), noise.to(DEV), torch.rand(T, d, dtype=torch.float64, generator=g).to(DEV)
        out = {}
        for name in ("coupled", "box"):
            acq, seeds = _nan(T), torch.full_like(md, float("nan"))
            kw = dict(seeds=seeds, x=x, best_v=best[name][0], best_x=best[name][1])
            if name == "coupled":
                F.jes_mc_group_forward(md, nd, K, T, S, acq, **kw)
            else:
                F.jes_mc_box_forward(md, nd, K, T, S, acq, box_of_point=words, **kw)
            out[name] = (acq, seeds, best[name][0].clone(), best[name][1].clone())
        for a, b in zip(out["coupled"], out["box"]):
            assert torch.equal(_bits(a), _bits(b)), call
    assert bool(torch.isfinite(best["box"][0]).all())


@pytest.mark.parametrize("n_boxes,K,T,S", [(2, 4, 5, 4), (3, 2, 9, 1), (1, 63, 3, 2)])
def test_both_box_modes_reproduce_the_recorded_bits(n_boxes, K, T, S):
    """tests/golden/jes_kernels_bits.npz (tools/record_jes_pair_golden.py --fixture kernels): three consecutive calls of
    mobocmf_jes_mc_box_forward, all boxes and the selected box (blocks, tracked), recorded on an MI355X while the per-box and
    the coupled launch were two kernels.  The regenerated inputs are the stored ones bit for bit; then the all-box rows and
    the selected mode's acq, best_v and best_x after every call are; the selected mode's seeds are the recorded coupled seeds
    in the own box (P2) and +0.0 elsewhere."""
    import os

    import numpy as np
    from mobocmf_amd import functional as F
    golden = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jes_kernels_bits.npz"))
    d = 3
    g = torch.Generator().manual_seed(T)
    box = RB.box_patterns(n_boxes, T)["blocks"]
    own = (torch.arange(n_boxes * (1 + K))[:, None] // (1 + K) == box[None, :].long())
    own = own[:, None, :, None].expand(n_boxes * (1 + K), 2, T, S).reshape(n_boxes * (1 + K), 2, T * S)
    best_v = torch.full((T,), float("-inf"), dtype=torch.float64, device=DEV)
    best_x = torch.zeros(T, d, dtype=torch.float64, device=DEV)
    for call in range(3):
        rec = lambda name: torch.from_numpy(golden["%d_%d_%d_%d/%d/%s" % (n_boxes, K, T, S, call, name)].copy())
        mom, noise = R.mc_inputs(n_boxes, K, T, S, seed=50 + call, flip=call)
        x = torch.rand(T, d, dtype=torch.float64, generator=g)
        for name, t in (("moments", mom), ("noise", noise), ("x", x)):
            assert torch.equal(_bits(t), rec(name)), (name, call)
        md, nd = mom.to(DEV), noise.to(DEV)
        rows, acq, seeds = _nan(n_boxes, T), _nan(T), torch.full_like(md, float("nan"))
        F.jes_mc_box_forward(md, nd, K, T, S, rows)
        F.jes_mc_box_forward(md, nd, K, T, S, acq, box_of_point=box.to(DEV), seeds=seeds, x=x.to(DEV), best_v=best_v,
                             best_x=best_x)
        for name, got in (("rows", rows), ("box_acq", acq), ("box_best_v", best_v), ("box_best_x", best_x)):
            assert torch.equal(_bits(got), rec(name)), (name, call)
        s = _bits(seeds)
        assert torch.equal(s[own], rec("seeds")[own]) and bool((s[~own] == 0).all()), call


def test_out_of_range_word_gives_nan_zero_seeds_and_no_tracking():
    from mobocmf_amd import functional as F
    n_boxes, K, T, S, d = 2, 2, 9, 3, 2
    mom, noise = R.mc_inputs(n_boxes, K, T, S, seed=6, flip=2)
    box = torch.tensor([0, 1, 2, -1, 1, 0, 1 << 30, 1, -(1 << 31)], dtype=torch.int32)
    bad = (box < 0) | (box >= n_boxes)
    x = torch.rand(T, d, dtype=torch.float64, generator=torch.Generator().manual_seed(1)).to(DEV)
    best_v = torch.full((T,), float("-inf"), dtype=torch.float64, device=DEV)
    best_x = torch.full((T, d), -7.0, dtype=torch.float64, device=DEV)
    acq, seeds = torch.zeros(T, dtype=torch.float64, device=DEV), _nan(*mom.shape)
    F.jes_mc_box_forward(mom.to(DEV), noise.to(DEV), K, T, S, acq, box_of_point=box.to(DEV), seeds=seeds, x=x, best_v=best_v,
                         best_x=best_x)
    torch.cuda.synchronize()
    acq_ref, seeds_ref, sc = RB.jes_mc_box_selected(mom, noise, K, T, S, box)
    a = acq.cpu()
    assert torch.equal(torch.isnan(a), bad) and bool(((a - acq_ref).abs()[~bad] <= 1e-14 * (1.0 + sc[~bad])).all())
    cols = bad[:, None].expand(T, S).reshape(T * S)
    assert bool((_bits(seeds)[:, :, cols] == 0).all())
    assert float((seeds.cpu() - seeds_ref).abs().max()) <= 1e-12 * float(seeds_ref.abs().max())
    assert bool((best_v.cpu()[bad] == float("-inf")).all()) and bool((best_x.cpu()[bad] == -7.0).all())
    assert torch.equal(_bits(best_v)[~bad], _bits(acq)[~bad]) and torch.equal(best_x.cpu()[~bad], x.cpu()[~bad])


def test_jes_mc_box_forward_refuses_bad_arguments():
    from mobocmf_amd import _lib
    from mobocmf_amd import functional as F
    z = lambda *s: torch.ones(*s, dtype=torch.float64, device=DEV)
    words = torch.zeros(4, dtype=torch.int32, device=DEV)
    T = 4
    with pytest.raises(_lib.MobocmfError):
        F.jes_mc_box_forward(z(4, 2, T), z(4), 0, T, 1, z(T), box_of_point=words)              # K = 0
    with pytest.raises(_lib.MobocmfError):
        F.jes_mc_box_forward(z(66, 2, T), z(66), 2, T, 1, z(T), box_of_point=words)            # 22 x 3 models = 66 > 64
    with pytest.raises(_lib.MobocmfError):
        F.jes_mc_box_forward(z(5, 2, T), z(5), 2, T, 1, z(T), box_of_point=words)              # not a multiple of 1 + K
    with pytest.raises(_lib.MobocmfError):
        F.jes_mc_box_forward(z(6, 2, T), z(6), 2, T, 1, z(2, T), seeds=z(6, 2, T))             # all boxes: no seeds
    with pytest.raises(_lib.MobocmfError):
        F.jes_mc_box_forward(z(6, 2, T), z(6), 2, T, 1, z(2, T), x=z(T, 2), best_v=z(T), best_x=z(T, 2))      # ... no tracking
    short = torch.as_strided(z(2 * T), (2, T), (T - 1, 1))
    with pytest.raises(_lib.MobocmfError):
        F.jes_mc_box_forward(z(6, 2, T), z(6), 2, T, 1, short)                                 # acq_ld = T - 1 < T
    with pytest.raises(_lib.MobocmfError):
        F.jes_mc_box_forward(z(6, 2, T), z(6), 2, T, 1, z(T), box_of_point=words.long())       # the words are int32
    rows = z(32, T)
    F.jes_mc_box_forward(z(64, 2, T), z(64), 1, T, 1, rows)                                    # 64 models: the most
    F.jes_mc_box_forward(z(64, 2, T), z(64), 63, T, 1, z(T), box_of_point=words)
    torch.cuda.synchronize()
    assert float(rows.abs().max()) == 0.0
