#!/usr/bin/env python3
"""CPU check of tests/test_gpu_staged_step.py's hand-placed starts: for every equation and
horizon of that test, roll its 70 starts out with the float64 oracle (oracle/equations.py,
adaptive scheme, the test's dw-from-memory stream) and report which of the four kinds of
trajectory the result holds.  Exits non-zero if a kind is missing anywhere.

    python tools/check_staged_starts.py
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import equations as oeq  # noqa: E402
from tests import test_gpu_staged_step as ts  # noqa: E402
from tests.helpers import eqn_config  # noqa: E402


def main():
    bad = 0
    B = ts.BATCHES[0]
    for name, d in ts.EQUATIONS:
        for N in ts.HORIZONS:
            eo = oeq.make(eqn_config(name, d, T=ts.T_TOTAL, N=N))
            x0, dw = ts.start_points(d, N, B), ts.host_dw(d, N, B)
            xr, dtr, cr = eo.propagate_adaptive(B, x0, dw, None, False, ts.T_TOTAL, N, True)
            got = ts.kinds(xr.permute(2, 0, 1), dtr, cr, N, torch.float64)
            ok = all(got.values())
            bad += not ok
            print(f"{name:8s} d={d:2d} N={N:3d}: {'ok ' if ok else 'MISSING'} {got if not ok else ''}")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
