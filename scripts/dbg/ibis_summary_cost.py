"""What per-period summaries of an IBIS run cost, in one process and session -> profiles/ibis_summary_cost.log.
For M in {512, 2^16, 2^20} parameter particles, T = 200 observations, chain 3, the README prior, microseconds per observation of
  (a) off        smc2 + smc2_run(ibis, window=16)
  (b) on         the same with summaries=[0.05, 0.5, 0.95], ahead=1: recorded inside the window launches
  (c) read-back  smc2_step per observation, then x, Sigma, theta, logw read from the device and reduced in numpy - what a trend
                 line cost before
alternating, 2 warm-up rounds and 7 timed rounds (host clock; every call ends in a device synchronise): median [min .. max].
A tree without the feature (SMC_ROOT pointing at it) times (a) alone: the figure (a) is compared with.
`--resources` (needs hipcc, no GPU): registers, scratch and occupancy of the window and summary kernels."""
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.environ.get("SMC_ROOT") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)


def resources():
    csrc = os.path.join(ROOT, "sequential_monte_carlo_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        out = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math", "-fPIC",
                              "-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.path.join(tmp, "ibis.o"), "smc_ibis.hip"],
                             cwd=csrc, capture_output=True, text=True).stderr
    name, row = None, {}
    print("kernel resource use (hipcc -Rpass-analysis=kernel-resource-usage, gfx950):")
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name, row = m.group(1), {}
        for key in ("VGPRs", "SGPRs Spill", "VGPRs Spill", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]"):
            m = re.search(r"remark:\s+" + re.escape(key) + r": (\d+)", line)
            if m and name:
                row[key] = int(m.group(1))
        if name and len(row) == 5 and re.search(r"k_ibis_(window|sum)", name):
            short = re.sub(r"^_ZN3smc\d+", "", name)[:30]
            print("  %-32s VGPRs %3d  scratch %3d B/lane  VGPR spills %d  SGPR spills %3d  occupancy %d waves/SIMD" % (
                short, row["VGPRs"], row["ScratchSize [bytes/lane]"], row["VGPRs Spill"], row["SGPRs Spill"], row["Occupancy [waves/SIMD]"]))
            name = None


if "--resources" in sys.argv:
    resources()
    sys.exit(0)

import numpy as np
import sequential_monte_carlo_amd as smc

T, CHAIN = 200, 3
_, y = smc.simulate(smc.UnivariateLinearGaussian(A=0.5, B=1.0, Q=0.9, R=0.8), T, seed=1998)
prior = smc.product_distribution([smc.TruncatedNormal(0, 1, -1, 1), smc.LogNormal(0, 1), smc.LogNormal(0, 1)])
tmap = smc.ThetaMap(1, [0, -1, 1, 2, -1, -1], [0.0, 1.0, 0.0, 0.0, 0.0, 1.0])
HAVE = hasattr(smc, "observation_dist")


def mod(th):
    return smc.UnivariateLinearGaussian(A=th[0], B=1.0, Q=th[1], R=th[2])


def fresh(ib, theta0, M):
    ib._handle().set_theta(theta0)
    ib.t, ib.n_rejuvenations, ib.ess = 0, 0, float(M)


def run_off(ib):
    smc.smc2(ib, y)
    smc.smc2_run(ib, y, 2, T, window=16, verbose=False)


def run_on(ib):
    ib.set_summaries([0.05, 0.5, 0.95], 1)
    smc.smc2(ib, y)
    smc.smc2_run(ib, y, 2, T, window=16, verbose=False)
    ib.set_summaries(None)
    assert len(ib.summary_trace) == T


def run_readback(ib):
    trend = []
    for t in range(1, T + 1):
        smc.smc2(ib, y) if t == 1 else smc.smc2_step(ib, y, t, verbose=False)
        x, S, th, lw = ib.x, ib.Sigma, ib.theta, ib.logw
        w = np.exp(lw - lw.max())
        w /= w.sum()
        ym, vm = th[:, 0] * x, th[:, 0] ** 2 * S + th[:, 1]
        trend.append((w @ ym, w @ vm))
    return trend


def med(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


print("IBIS summaries cost, T = %d, chain %d, README prior; us per observation, host clock; tree %s the feature" % (T, CHAIN, "with" if HAVE else "WITHOUT"))
for M in (512, 1 << 16, 1 << 20):
    ib = smc.IBIS(M, mod, prior, CHAIN, 0.5, seed=3, theta_map=tmap)
    theta0 = ib.theta
    configs = [("(a) off", run_off)] + ([("(b) on", run_on), ("(c) read-back", run_readback)] if HAVE else [])
    ts = {name: [] for name, _ in configs}
    for rep in range(9):
        for name, f in configs:
            fresh(ib, theta0, M)
            t0 = time.perf_counter()
            f(ib)
            if rep >= 2:
                ts[name].append((time.perf_counter() - t0) * 1e6 / T)
    for name, _ in configs:
        print("M = %7d   %-14s %10.2f us/observation [%10.2f ..%10.2f]   rejuvenations %d" % ((M, name) + med(ts[name]) + (ib.n_rejuvenations,)), flush=True)
    ib.close()
