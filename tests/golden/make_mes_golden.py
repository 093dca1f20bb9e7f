"""Writes tests/golden/mes_kernel_cases.npz: the inputs of the MES kernel test (tests/mes_reference.py mes_case, the shapes
MES_SHAPES) and, from mpmath at 50 digits, acq, the seeds, kappa = 1 / (1 - cdf) per objective and point, whether the cdf clamp
binds there, and the unclamped term.  Numbers only.  Run from the repository root:  python tests/golden/make_mes_golden.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import mes_reference as M      # noqa: E402


def build():
    out = {}
    for shape in M.MES_SHAPES:
        c = M.mes_case(*shape)
        acq, seeds, kappa, clamped, term = M.mes_mp(c)
        p = "o%d_c%d_T%d_" % shape
        out.update({p + "moments": c["moments"], p + "noise": c["noise"], p + "best": c["best"], p + "acq": acq, p + "seeds": seeds,
                    p + "kappa": kappa, p + "clamped": clamped, p + "term": term})
    return out


if __name__ == "__main__":
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mes_kernel_cases.npz")
    np.savez(path, **build())
    print("wrote", path)
