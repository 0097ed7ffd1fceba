"""What the per-step summaries cost per summary mode: no summaries | weighted | unweighted (smc_set_summary_mode), three levels with
and without moments.  Shapes: LDS-resident filters of 1024 and 8192 particles (1000 steps), multi-segment filters of 2^20 and 2^22
(300 steps).  Every cell: 2 warm-up calls, then 7 timed calls (host clock around a call that ends in a synchronise); median
[min .. max] in microseconds per step.  A library without the mode (an older build, for comparison) prints the first two columns."""
import os
import sys
import time

sys.path.insert(0, os.environ.get("SMC_ROOT") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import numpy as np
import sequential_monte_carlo_amd as smc
from sequential_monte_carlo_amd import _lib as L

LGR = [0.5, 1.0, 0.9, 0.8, 0.0, 1.0]
PS = [0.25, 0.5, 0.75]
label = sys.argv[1] if len(sys.argv) > 1 else "build"
m = smc.UnivariateLinearGaussian(A=0.5, B=1.0, Q=0.9, R=0.8)
has_mode = hasattr(L.Handle, "set_summary_mode")


def cell(h, y):
    for _ in range(2):
        h.log_likelihood(y)
    ts = []
    for _ in range(7):
        t0 = time.perf_counter()
        h.log_likelihood(y)
        ts.append((time.perf_counter() - t0) * 1e6 / len(y))
    ts.sort()
    return "%7.2f [%7.2f ..%7.2f]" % (ts[3], ts[0], ts[-1])


for nth, n, T in ((1, 1024, 1000), (512, 1024, 1000), (1, 8192, 1000), (1, 1 << 20, 300), (1, 1 << 22, 300)):
    _, y = smc.simulate(m, T)
    h = L.Handle(1, nth, n, seed=3)
    h.set_params(np.tile(LGR, (nth, 1)))
    h.set_summaries()
    print("%s n_theta=%d Nx=%d %-18s none %s" % (label, nth, n, "-", cell(h, y)), flush=True)
    for name, mom in (("3 levels", False), ("3 levels + moments", True)):
        row = []
        for mode in ("weighted", "unweighted") if has_mode else ("weighted",):
            if has_mode:
                h.set_summary_mode(mode)
            h.set_summaries(PS, 0, moments=mom)
            row.append("%s %s" % (mode, cell(h, y)))
        print("%s n_theta=%d Nx=%d %-18s %s" % (label, nth, n, name, "  ".join(row)), flush=True)
    h.close()
