#!/usr/bin/env python3
"""Records tests/golden/frozen_layer_bits.npz: the bit patterns of a layer's frozen CHAIN state and of the PANEL calls against
it (functional.freeze_chain, layer_panel_frozen and its backward, predictive_covariance), and of a three-layer model's
predict_for_acquisition and its dX inside MFDGP.frozen_chains().  tests/frozen_layer_cases.py holds the calls and the key
names; tests/test_hip_layer.py and tests/test_hip_overlap.py compare against the file with torch.equal.

The committed fixture was recorded on an MI355X at commit 591b8f6 ("Evolve sampled Pareto sets on the GPU: NSGA-II over chain
samples"), the last one where the frozen path ran through the phase field of the layer descriptor (a CHAIN-only call into a `saved`
buffer, the state copied to the front of a fresh `saved` per PANEL call).  The tool goes through calls that exist on both
sides of that change: at a later commit it records whatever they compute there.

usage: python tools/record_frozen_layer_golden.py [--out FILE.npz]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import numpy as np
    from tests import frozen_layer_cases as C
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "frozen_layer_bits.npz"))
    a = ap.parse_args()
    out, after = C.layer_arrays()
    for k, v in after.items():
        assert (out[k] == v).all(), "a PANEL call wrote into the frozen state: " + k
    out.update(C.model_arrays())
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **{k: v.numpy() for k, v in out.items()})
    print("wrote", a.out, os.path.getsize(a.out), "bytes,", len(out), "arrays")
    return 0


if __name__ == "__main__":
    sys.exit(main())
