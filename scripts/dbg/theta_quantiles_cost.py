"""What the quantiles and histograms of the theta cloud cost on the device, in one process -> profiles/theta_quantiles_cost.log.
For M in {512, 2^16, 2^20} parameter particles and d in {1, 3, 8}, random theta and log-weights on a handle, alternating in one
session, 3 warm-up and 9 timed rounds each (host clock; every call ends in a device synchronise), median [min .. max] in ms:
  quantiles   smc_ibis_theta_quantiles at three levels (0.05, 0.5, 0.95)
  histogram   smc_ibis_theta_histogram, 50 bins of coordinate 0
  moments     smc_ibis_theta_moments (weighted): the floor of a reduction over the same bytes
  readback    what the parent commit offers: smc_ibis_get of theta and logw ...
  +numpy      ... and numpy's sort-based weighted quantile of every coordinate on them (argsort, cumsum, searchsorted)
bytes: what the kernels of a quantiles call read, 8 M for k_ibis_kmax, 16 M for k_theta_weights (logw in, q out) and per pass
8 M (q) + 64 M (the rows of theta are padded to 8 doubles) - and the rate that makes of the call's time, against the 6.29 TB/s a
copy reaches on the MI355X (8 TB/s nominal).  A whole-call rate: launches, the picks and the synchronise are inside it.
`--trace` runs 20 quantile calls at the largest size and d = 3 only (for a kernel trace of the passes, taken in a run of its own)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)

from sequential_monte_carlo_amd import _lib as L  # noqa: E402

P = np.array([0.05, 0.5, 0.95])
SIZES = [int(a) for a in sys.argv[1:] if a.isdigit()] or [512, 1 << 16, 1 << 20]
PASSES, HBM = 8, 6.29e12


def med(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def handle(M, d, rng):
    fam = np.full(d, L.PRIOR_NORMAL, dtype=np.int32)
    par = np.tile([0.0, 1.0, 0.0, 0.0, 0.0], (d, 1))
    h = L.IbisHandle(M, d, fam, par, [0, -1, -1, -1, -1, -1], [0.0, 1.0, 0.9, 0.8, 0.0, 1.0])
    h.set_theta(rng.normal(size=(M, d)))
    h.set_logw(3.0 * rng.normal(size=M))
    return h


def numpy_quantiles(theta, logw):
    w = np.exp(logw - logw.max())
    out = np.zeros((theta.shape[1], P.size))
    for i in range(theta.shape[1]):
        idx = np.argsort(theta[:, i], kind="stable")
        cum = np.cumsum(w[idx])
        out[i] = theta[idx[np.minimum(np.searchsorted(cum, P * cum[-1], side="right"), idx.size - 1)], i]
    return out


if "--trace" in sys.argv:
    h = handle(max(SIZES), 3, np.random.default_rng(1))
    for _ in range(20):
        h.theta_quantiles(P)
    h.close()
    sys.exit(0)

print("theta quantiles and histograms: ms per call, median [min .. max] of 9 rounds, 3 levels, 50 bins")
for M in SIZES:
    for d in (1, 3, 8):
        h = handle(M, d, np.random.default_rng(M + d))
        got = {}

        def readback():
            got["s"] = h.get(theta=True, logw=True)

        calls = (("quantiles", lambda: h.theta_quantiles(P)), ("histogram", lambda: h.theta_histogram(0, -4.0, 4.0, 50)),
                 ("moments", lambda: h.theta_moments(True)), ("readback", readback),
                 ("+numpy", lambda: numpy_quantiles(got["s"]["theta"], got["s"]["logw"])))
        ts = {name: [] for name, _ in calls}
        for rep in range(12):
            for name, call in calls:
                t0 = time.perf_counter()
                call()
                if rep >= 3:
                    ts[name].append((time.perf_counter() - t0) * 1e3)
        q = h.theta_quantiles(P)
        s = h.get(theta=True, logw=True)
        assert np.array_equal(q, L.host_theta_quantiles(s["theta"], s["logw"], P))
        nbytes = 8 * M + 16 * M + PASSES * (8 + 64) * M
        for name, _ in calls:
            m = med(ts[name])
            extra = ""
            if name == "quantiles":
                extra = "   %6.1f MB read, %7.1f GB/s = %4.1f %% of the copy rate" % (nbytes / 1e6, nbytes / m[0] / 1e6, 100.0 * nbytes / (m[0] * 1e-3) / HBM)
            if name == "readback":
                extra = "   %6.1f MB over the bus (the rows of theta cross it padded to 8 doubles)" % (8 * (8 + 1) * M / 1e6)
            print("M = %7d  d = %d  %-10s %9.3f ms [%9.3f ..%9.3f]%s" % ((M, d, name) + m + (extra,)), flush=True)
        h.close()
