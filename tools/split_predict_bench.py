#!/usr/bin/env python3
"""The launches of the frozen-chain predict groups on their own (util/panel_predict.py), six untrained models of d = 2, S = 25,
chains frozen: scoring the raw candidates of a search (T = 200, one MOBOCMF_STEP_FORWARD launch) and the two model evaluations
of an iterate (T = 5), per fidelity, through SplitPredictGroup at M = 640 and 1024 and through both groups at M = 512.  A host
clock around a synchronise; [median, largest minus smallest] in microseconds.  One JSON line per (M, group).

usage: python tools/split_predict_bench.py
"""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mobocmf_amd import _lib
from mobocmf_amd.util import synthetic
from mobocmf_amd.util.panel_predict import PanelPredictGroup, SplitPredictGroup
from tests.test_hip_model import build_model

def timed(fn, n):
    fn()      # (the first call per device and mode sets the kernel's attribute)
    ts = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return round(1e6 * statistics.median(ts), 1), round(1e6 * (max(ts) - min(ts)), 1)

for M, kinds in ((512, (PanelPredictGroup, SplitPredictGroup)), (640, (SplitPredictGroup,)), (1024, (SplitPredictGroup,))):
    models = [build_model(synthetic.make_problem(d=2, L=2, M=M, N=M, S=25, seed=40 + i), S_train=1, S_acq=25) for i in range(6)]
    for kind in kinds:
        out = {"M": M, "group": kind.__name__}
        for f in (0, 1):
            raw = kind(models, f, 200, 2, want_gradients=False)
            it = kind(models, f, 5, 2)
            g = torch.Generator().manual_seed(M)
            raw.x.copy_(torch.rand(200, 2, dtype=torch.float64, generator=g))
            it.x.copy_(torch.rand(5, 2, dtype=torch.float64, generator=g))
            it.seeds.copy_(torch.randn(*it.seeds.shape, dtype=torch.float64, generator=g))
            with raw.frozen(), it.frozen():
                out["raw_forward_us_f%d" % f] = timed(lambda: raw._launch(_lib.STEP_FORWARD), 7)
                out["iterate_forward_us_f%d" % f] = timed(lambda: it._launch(_lib.STEP_FORWARD), 21)
                out["iterate_gradient_us_f%d" % f] = timed(lambda: it._launch(_lib.STEP_INPUT_GRADIENTS), 21)
        print(json.dumps(out), flush=True)
