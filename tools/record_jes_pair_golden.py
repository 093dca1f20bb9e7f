#!/usr/bin/env python3
"""Records the two bitwise fixtures of the JES launches (csrc/acq_search.hip).

--fixture pair: tests/golden/jes_pair_kernel_bits.npz, what the one-thread-per-test-point JES kernel (jes_group_kernel, behind
mobocmf_jes_group_forward) computed before it was retired in favour of jes_mc_group_kernel at K = 1.  The committed fixture
was recorded on an MI355X at commit b1f2b51 ("Average the JES acquisition over K sampled Pareto sets"), the last one that has
that kernel; run at a later commit this tool records whatever mobocmf_jes_group_forward launches there.

Per shape (n_pairs, T, S) three consecutive calls of functional.jes_group_forward with seeds, x, best_v and best_x, the
tracking carried from call to call, on tests/jes_mc_reference.mc_inputs(n_pairs, 1, T, S, seed=30 + call, flip=call).  Inputs
(moments, noise, x) and outputs (acq, seeds, best_v, best_x after each call) are stored as int64 bit patterns under the keys
"<n_pairs>_<T>_<S>/<call>/<name>".  tests/test_hip_jes_mc.py::test_one_sample_reproduces_the_recorded_pair_kernel reads it.

--fixture kernels (the default): tests/golden/jes_kernels_bits.npz, what mobocmf_jes_mc_group_forward and
mobocmf_jes_mc_box_forward computed while they launched two kernels kept equal by hand (jes_mc_group_kernel,
jes_mc_box_kernel), before those became the modes of one.  The committed fixture was recorded on an MI355X at commit d6d33d6
("Decoupled evaluations: per-black-box JES search on host and device"), the last one with two kernels.  The tool goes through
functional.jes_mc_group_forward / jes_mc_box_forward alone: at a later commit it records whatever those launch there.

Per shape (n_boxes, K, T, S) three consecutive calls on mc_inputs(n_boxes, K, T, S, seed=50 + call, flip=call), x drawn from
a CPU generator seeded with T, best_v starting at -inf, under "<n_boxes>_<K>_<T>_<S>/<call>/<name>": the inputs moments, noise,
x; the coupled entry point's acq, seeds, best_v, best_x; the all-box mode's rows (n_boxes, T); the selected-box mode's box_acq,
box_best_v, box_best_x with jes_box_reference.box_patterns(n_boxes, T)["blocks"], its tracking its own.  (The selected-box
seeds are not stored: P2 of include/mobocmf_hip.h ties them to the coupled seeds, tests/test_hip_jes_box.py checks that.)
tests/test_hip_jes_mc.py and tests/test_hip_jes_box.py read it.

usage: python tools/record_jes_pair_golden.py [--fixture pair|kernels] [--out FILE.npz]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((3, 5, 4), (2, 67, 1), (32, 3, 2))      # (32, 3, 2): 64 models, every lane of the wavefront busy
# (n_boxes, K, T, S): several boxes with K > 1; S = 1; (1, 63, 3, 2): 64 models, every lane busy
KERNEL_SHAPES = ((2, 4, 5, 4), (3, 2, 9, 1), (1, 63, 3, 2))
CALLS, D = 3, 3
FILES = {"pair": "jes_pair_kernel_bits.npz", "kernels": "jes_kernels_bits.npz"}


def record_pair(torch, F, R, bits):
    out = {}
    for n_pairs, T, S in SHAPES:
        g = torch.Generator().manual_seed(T)
        best_v = torch.full((T,), float("-inf"), dtype=torch.float64, device="cuda")
        best_x = torch.zeros(T, D, dtype=torch.float64, device="cuda")
        for call in range(CALLS):
            mom, noise = R.mc_inputs(n_pairs, 1, T, S, seed=30 + call, flip=call)
            x = torch.rand(T, D, dtype=torch.float64, generator=g)
            md = mom.cuda()
            acq, seeds = torch.zeros(T, dtype=torch.float64, device="cuda"), torch.full_like(md, float("nan"))
            F.jes_group_forward(md, noise.cuda(), T, S, acq, seeds=seeds, x=x.cuda(), best_v=best_v, best_x=best_x)
            torch.cuda.synchronize()
            for name, t in dict(moments=mom, noise=noise, x=x, acq=acq, seeds=seeds, best_v=best_v, best_x=best_x).items():
                out["%d_%d_%d/%d/%s" % (n_pairs, T, S, call, name)] = bits(t)
    return out


def record_kernels(torch, F, R, bits):
    from tests import jes_box_reference as RB
    out = {}
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float64, device="cuda")
    for n_boxes, K, T, S in KERNEL_SHAPES:
        g = torch.Generator().manual_seed(T)
        words = RB.box_patterns(n_boxes, T)["blocks"].cuda()
        best = [(torch.full((T,), float("-inf"), dtype=torch.float64, device="cuda"),
                 torch.zeros(T, D, dtype=torch.float64, device="cuda")) for _ in range(2)]      # coupled; selected box
        for call in range(CALLS):
            mom, noise = R.mc_inputs(n_boxes, K, T, S, seed=50 + call, flip=call)
            x = torch.rand(T, D, dtype=torch.float64, generator=g)
            md, nd, xd = mom.cuda(), noise.cuda(), x.cuda()
            acq, seeds, rows, box_acq = nan(T), torch.full_like(md, float("nan")), nan(n_boxes, T), nan(T)
            F.jes_mc_group_forward(md, nd, K, T, S, acq, seeds=seeds, x=xd, best_v=best[0][0], best_x=best[0][1])
            F.jes_mc_box_forward(md, nd, K, T, S, rows)
            F.jes_mc_box_forward(md, nd, K, T, S, box_acq, box_of_point=words, seeds=torch.full_like(md, float("nan")), x=xd,
                                 best_v=best[1][0], best_x=best[1][1])
            torch.cuda.synchronize()
            for name, t in dict(moments=mom, noise=noise, x=x, acq=acq, seeds=seeds, best_v=best[0][0], best_x=best[0][1],
                                rows=rows, box_acq=box_acq, box_best_v=best[1][0], box_best_x=best[1][1]).items():
                out["%d_%d_%d_%d/%d/%s" % (n_boxes, K, T, S, call, name)] = bits(t)
    return out


def main():
    import numpy as np
    import torch
    from mobocmf_amd import functional as F
    from tests import jes_mc_reference as R
    ap = argparse.ArgumentParser()
    ap.add_argument("--fixture", choices=sorted(FILES), default="kernels")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    path = a.out or os.path.join(ROOT, "tests", "golden", FILES[a.fixture])
    bits = lambda t: t.detach().cpu().contiguous().view(torch.int64).numpy().copy()
    out = (record_pair if a.fixture == "pair" else record_kernels)(torch, F, R, bits)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(out), "arrays")
    return 0


if __name__ == "__main__":
    sys.exit(main())
