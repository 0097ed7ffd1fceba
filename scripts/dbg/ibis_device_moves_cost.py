"""What IBIS(..., device_moves=True) buys, in one process and session -> profiles/ibis_device_moves.log (a sibling of
ibis_cost.py).  For M in {512, 2^16, 2^20} parameter particles, T = 200 observations, chain 3, the README prior:
  online   microseconds per observation of smc2 + smc2_run(ibis, ..., window=16), device_moves False against True, alternating,
           2 warm-up runs and 7 timed runs each (host clock; every call ends in a device synchronise): median [min .. max]
  move     one resample_ + rejuvenate_ on the filtered cloud at M = 2^20, both ways, the same protocol, in ms
  parts    the device calls of a move alone at M = 2^20 (resample, theta_moments unweighted / weighted): their fixed cost,
           the serial left-to-right combines and the one-workgroup scan of the tile sums included
SMC_ROOT=<a built checkout of another commit> with --default-only runs the default path of that checkout (the parent commit's
figure for False: it has no flag)."""
import os
import sys
import time

ROOT = os.environ.get("SMC_ROOT") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)

import sequential_monte_carlo_amd as smc  # noqa: E402

T, CHAIN = 200, 3
_, y = smc.simulate(smc.UnivariateLinearGaussian(A=0.5, B=1.0, Q=0.9, R=0.8), T, seed=1998)
prior = smc.product_distribution([smc.TruncatedNormal(0, 1, -1, 1), smc.LogNormal(0, 1), smc.LogNormal(0, 1)])
tmap = smc.ThetaMap(1, [0, -1, 1, 2, -1, -1], [0.0, 1.0, 0.0, 0.0, 0.0, 1.0])
PARENT = "--default-only" in sys.argv          # a build without the new entry points: the default path alone
FLAGS = (False,) if PARENT else (False, True)
SIZES = [int(a) for a in sys.argv[1:] if a.isdigit()] or [512, 1 << 16, 1 << 20]


def mod(th):
    return smc.UnivariateLinearGaussian(A=th[0], B=1.0, Q=th[1], R=th[2])


def med(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def sampler(M, flag):
    kw = {"device_moves": True} if flag else {}
    return smc.IBIS(M, mod, prior, CHAIN, 0.5, seed=3, theta_map=tmap, **kw)


print("IBIS device moves, T = %d, chain %d, README prior, window 16%s" % (T, CHAIN, "  [default path of the checkout SMC_ROOT]" if PARENT else ""))
for M in SIZES:
    ibs = {f: sampler(M, f) for f in FLAGS}
    ts = {f: [] for f in FLAGS}
    for rep in range(9):
        for f in FLAGS:
            ib = ibs[f]
            ib._handle().set_theta(ib._theta0)
            ib.t, ib.n_rejuvenations, ib.ess, ib._calls = 0, 0, float(M), 0
            t0 = time.perf_counter()
            smc.smc2(ib, y)
            smc.smc2_run(ib, y, 2, T, window=16, verbose=False)
            if rep >= 2:
                ts[f].append((time.perf_counter() - t0) * 1e6 / T)
    for f in FLAGS:
        print("online  M = %7d  device_moves=%-5s %9.2f us/observation [%9.2f ..%9.2f]   rejuvenations %d  E[A] %.6f" % (
            (M, f) + med(ts[f]) + (ibs[f].n_rejuvenations, smc.expected_parameters(ibs[f])[0])), flush=True)
    if M == max(SIZES):
        ts = {f: [] for f in FLAGS}
        for rep in range(9):
            for f in FLAGS:
                ib = ibs[f]
                ib._handle().set_theta(ib._theta0)
                ib._handle().filter(y)
                t0 = time.perf_counter()
                smc.resample_(ib)
                smc.rejuvenate_(ib, y)
                if rep >= 2:
                    ts[f].append((time.perf_counter() - t0) * 1e3)
        for f in FLAGS:
            print("move    M = %7d  device_moves=%-5s %9.3f ms per resample_ + rejuvenate_ [%9.3f ..%9.3f]   acc %.3f" % (
                (M, f) + med(ts[f]) + (ibs[f].acc_ratio,)), flush=True)
    if M == max(SIZES) and not PARENT:
        h = ibs[True]._handle()
        h.set_theta(ibs[True]._theta0)
        h.filter(y)
        for name, call in (("resample", lambda: h.resample(12345)), ("theta_moments(unweighted)", lambda: h.theta_moments(False)),
                           ("theta_moments(weighted)", lambda: h.theta_moments(True))):
            tp = []
            for rep in range(9):
                t0 = time.perf_counter()
                call()
                if rep >= 2:
                    tp.append((time.perf_counter() - t0) * 1e3)
            print("parts   M = %7d  %-26s %9.3f ms [%9.3f ..%9.3f]" % ((M, name) + med(tp)), flush=True)
    for ib in ibs.values():
        ib.close()
