#!/usr/bin/env python3
"""Records tests/golden/jes_pair_kernel_bits.npz: what the one-thread-per-test-point JES kernel (jes_group_kernel, behind
mobocmf_jes_group_forward) computed before it was retired in favour of jes_mc_group_kernel at K = 1.  The committed fixture
was recorded on an MI355X at commit b1f2b51 ("Average the JES acquisition over K sampled Pareto sets"), the last one that has
that kernel; run at a later commit this tool records whatever mobocmf_jes_group_forward launches there.

Per shape (n_pairs, T, S) three consecutive calls of functional.jes_group_forward with seeds, x, best_v and best_x, the
tracking carried from call to call, on tests/jes_mc_reference.mc_inputs(n_pairs, 1, T, S, seed=30 + call, flip=call).  Inputs
(moments, noise, x) and outputs (acq, seeds, best_v, best_x after each call) are stored as int64 bit patterns under the keys
"<n_pairs>_<T>_<S>/<call>/<name>".  tests/test_hip_jes_mc.py::test_one_sample_reproduces_the_recorded_pair_kernel reads it.

usage: python tools/record_jes_pair_golden.py [--out tests/golden/jes_pair_kernel_bits.npz]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((3, 5, 4), (2, 67, 1), (32, 3, 2))      # (32, 3, 2): 64 models, every lane of the wavefront busy
CALLS, D = 3, 3


def main():
    import numpy as np
    import torch
    from mobocmf_amd import functional as F
    from tests import jes_mc_reference as R
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "jes_pair_kernel_bits.npz"))
    a = ap.parse_args()
    bits = lambda t: t.detach().cpu().contiguous().view(torch.int64).numpy().copy()
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
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **out)
    print("wrote", a.out, os.path.getsize(a.out), "bytes,", len(out), "arrays")
    return 0


if __name__ == "__main__":
    sys.exit(main())
