#!/usr/bin/env python3
"""Build container: the largest absolute error of acos_defined (csrc/hlsl_math.hpp, restated in tests/line_common.py) against float64
acos, on 2^24 + 1 evenly spaced float32 inputs of [-1, 1] plus 2 x 10^5 log-spaced towards +1 and -1; numpy's float32 arccos on the same
set beside it.  The condition is 2^-21 (two ulp of the binade that holds pi).  No GPU needed.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests.line_common import acos_defined  # noqa: E402


def main():
    n = 1 << 24
    t = np.logspace(np.log10(2.0 ** -24), 0.0, 100000)
    worst, worst_numpy, where = 0.0, 0.0, 0.0
    pieces = [(np.arange(lo, min(lo + (1 << 20), n + 1), dtype=np.float64) / n * 2 - 1) for lo in range(0, n + 1, 1 << 20)] + [1 - t, -1 + t]
    for x in pieces:
        x = x.astype(np.float32)
        exact = np.arccos(x.astype(np.float64))
        err = np.abs(acos_defined(x).astype(np.float64) - exact)
        if err.max() > worst:
            worst, where = float(err.max()), float(x[err.argmax()])
        worst_numpy = max(worst_numpy, float(np.abs(np.arccos(x).astype(np.float64) - exact).max()))
    print("acos_defined: largest |error| %.4g at x = %r; numpy float32 arccos: %.4g; bound 2^-21 = %.4g" % (worst, where, worst_numpy, 2.0 ** -21))
    return 0 if worst <= 2.0 ** -21 else 1


if __name__ == "__main__":
    sys.exit(main())
