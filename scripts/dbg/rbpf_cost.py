"""What the marginal (Rao-Blackwellised) UCSV family costs and buys against bootstrap UCSV and OPTIMAL-guided UCSV, on one series
in one process and session (the log: profiles/rbpf_cost.log).
  time      512 filters x 1024 and 512 x 8192 particles, 300 steps: 2 warm-up calls, 7 timed calls (host clock around a call that
            ends in a synchronise); median [min .. max] in microseconds per step
  variance  var(logZ) over 256 independent filters (stream ids 0..255) at Nx = 256, 1024, 8192, T = 100, with its standard error
            sqrt(2 / (K - 1)) var; and, for the marginal family alone, at Nx = 16 .. 8192 (powers of two): the smallest Nx whose var(logZ) is at
            or below bootstrap UCSV's at 8192
Row (0.2, 0.2, 0, -1, -2) as profiles/guided_cost.log."""
import os
import sys
import time

sys.path.insert(0, os.environ.get("SMC_ROOT") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import numpy as np
from sequential_monte_carlo_amd import _lib as L

UCR = [0.2, 0.2, 0.0, -1.0, -2.0]
FAMILIES = (("bootstrap", L.MODEL_UCSV3D, L.PROP_NONE), ("guided", L.MODEL_UCSV3D, L.PROP_OPTIMAL), ("marginal", L.MODEL_UCSV_RB, L.PROP_NONE))


def handle(model, kind, nth, n, seed=3):
    h = L.Handle(model, nth, n, seed=seed)
    h.set_params(np.tile(UCR, (nth, 1)))
    if kind != L.PROP_NONE:
        h.set_proposal(kind)
    return h


_, y = L.simulate(L.MODEL_UCSV3D, UCR, 300, 1998)
for n in (1024, 8192):
    med = {}
    for rep in range(2):
        for label, model, kind in FAMILIES:
            h = handle(model, kind, 512, n)
            for _ in range(2):
                h.log_likelihood(y)
            ts = []
            for _ in range(7):
                t0 = time.perf_counter()
                h.log_likelihood(y)
                ts.append((time.perf_counter() - t0) * 1e6 / len(y))
            ts.sort()
            med.setdefault(label, []).append(ts[3])
            print("UCSV 512 x %-5d %-9s %8.2f [%8.2f ..%8.2f] us/step  (seg %d x %d, resident %d)" % (n, label, ts[3], ts[0], ts[-1], h.seg, h.nseg, h.resident), flush=True)
            h.close()
    print("UCSV 512 x %-5d time marginal / bootstrap %.3f, marginal / guided %.3f" % (
        n, np.mean(med["marginal"]) / np.mean(med["bootstrap"]), np.mean(med["marginal"]) / np.mean(med["guided"])), flush=True)

K, T = 256, 100
yv = y[:T]
var = {}
for n in (256, 1024, 8192):
    for label, model, kind in FAMILIES:
        h = handle(model, kind, K, n, seed=5)
        z = h.log_likelihood(yv)
        h.close()
        var[(label, n)] = float(np.var(z, ddof=1))
        print("var(logZ) K = %d, T = %d, Nx = %-5d %-9s %.5f +- %.5f   mean logZ %.4f" % (K, T, n, label, var[(label, n)], var[(label, n)] * np.sqrt(2.0 / (K - 1)), z.mean()), flush=True)
    print("var(logZ) Nx = %-5d marginal / bootstrap %.3f, marginal / guided %.3f" % (
        n, var[("marginal", n)] / var[("bootstrap", n)], var[("marginal", n)] / var[("guided", n)]), flush=True)
target = var[("bootstrap", 8192)]
smallest = None
for n in (16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 8192):
    h = handle(L.MODEL_UCSV_RB, L.PROP_NONE, K, n, seed=5)
    v = float(np.var(h.log_likelihood(yv), ddof=1))
    h.close()
    print("var(logZ) marginal Nx = %-5d %.5f   (bootstrap at 8192: %.5f)" % (n, v, target), flush=True)
    if smallest is None and v <= target:
        smallest = n
print("smallest Nx (powers of two) of the marginal family with var(logZ) <= bootstrap UCSV's at 8192: %s" % smallest, flush=True)
