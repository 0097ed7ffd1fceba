"""What the IBIS sampler's device path costs, in one process and session -> profiles/ibis_cost.log.
For M in {512, 2^16, 2^20} parameter particles, T = 200 observations, chain 3, the README prior:
  rejuvenate   rejuvenate_(ibis, y) - one fused launch (k_ibis_rejuvenate) plus the host's random-walk factor - against the
               composition the library offered before it: per chain position a host proposal, smc.log_likelihood_kalman's batched
               call on M rows (upload rows, download results) and a host accept, with the same random-walk factor.  Alternating,
               2 warm-up calls and 7 timed calls each (host clock; both end in a device synchronise): median [min .. max] in ms.
  online       microseconds per observation of smc2_run(ibis, ..., window=16), beside smc2_run of SMC(1024, 512) on the same y
               (context only: different estimators).
`--resources` (needs hipcc, no GPU): registers and scratch of the IBIS kernels from -Rpass-analysis=kernel-resource-usage."""
import io
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
    name = None
    print("kernel resource use (hipcc -Rpass-analysis=kernel-resource-usage, gfx950):")
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            row = {}
        for key in ("VGPRs", "SGPRs Spill", "VGPRs Spill", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]"):
            m = re.search(r"remark:\s+" + re.escape(key) + r": (\d+)", line)
            if m and name:
                row[key] = int(m.group(1))
                if key == "VGPRs Spill" and re.search(r"k_ibis_(window|rejuvenate|permute)", name):
                    dem = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip() or name
                    short = re.sub(r"\(.*", "", dem).replace("void smc::", "").replace("smc::", "")   # k_ibis_window<Lg1Row, true, false, false>
                    print("  %-44s VGPRs %3d  scratch %3d B/lane  VGPR spills %d  SGPR spills %3d  occupancy %d waves/SIMD" % (
                        short, row["VGPRs"], row["ScratchSize [bytes/lane]"], row["VGPRs Spill"], row["SGPRs Spill"], row["Occupancy [waves/SIMD]"]))


if "--resources" in sys.argv:
    resources()
    sys.exit(0)

import numpy as np
import sequential_monte_carlo_amd as smc
from sequential_monte_carlo_amd import _lib as L
from sequential_monte_carlo_amd.smc_samplers import random_walk_kernel

T, CHAIN = 200, 3
_, y = smc.simulate(smc.UnivariateLinearGaussian(A=0.5, B=1.0, Q=0.9, R=0.8), T, seed=1998)
prior = smc.product_distribution([smc.TruncatedNormal(0, 1, -1, 1), smc.LogNormal(0, 1), smc.LogNormal(0, 1)])
tmap = smc.ThetaMap(1, [0, -1, 1, 2, -1, -1], [0.0, 1.0, 0.0, 0.0, 0.0, 1.0])


def mod(th):
    return smc.UnivariateLinearGaussian(A=th[0], B=1.0, Q=th[1], R=th[2])


def composition(theta, logZ, rng):
    """rejuvenate! with the exact likelihood as the library could do it without the fused kernel"""
    theta, logZ = theta.copy(), logZ.copy()
    kernel = random_walk_kernel(theta)
    scales = 0.5 * np.arange(CHAIN, 0, -1)
    for c in range(CHAIN):
        prop = kernel.many(theta, scales[c], rng)
        u = rng.random(theta.shape[0])
        ok = prior.insupport_many(prop)
        safe = np.where(ok[:, None], prop, theta)
        lp_prop, lp_cur = prior.logpdf_many(safe), prior.logpdf_many(theta)
        z = L.kalman_log_likelihood(tmap.rows(safe), y)[:, 2]
        acc = ok & (z + lp_prop > -np.inf) & (np.log(u) < (z - logZ) + (lp_prop - lp_cur))
        theta[acc], logZ[acc] = prop[acc], z[acc]
    return theta, logZ


def med(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


print("IBIS cost, T = %d, chain %d, README prior (3 parameters); times are host clock around calls that end in a synchronise" % (T, CHAIN))
for M in (512, 1 << 16, 1 << 20):
    ib = smc.IBIS(M, mod, prior, CHAIN, 0.5, seed=3, theta_map=tmap)
    ib._handle().filter(y)
    theta0, logZ0 = ib.theta, ib.logZ
    rng = np.random.default_rng(1)
    tf, tc = [], []
    for rep in range(9):
        ib._handle().set_theta(theta0)
        ib._handle().filter(y)
        t0 = time.perf_counter()
        smc.rejuvenate_(ib, y)
        a = time.perf_counter() - t0
        t0 = time.perf_counter()
        composition(theta0, logZ0, rng)
        b = time.perf_counter() - t0
        if rep >= 2:
            tf.append(a * 1e3)
            tc.append(b * 1e3)
    f, c = med(tf), med(tc)
    print("rejuvenate M = %7d   fused %9.3f ms [%9.3f ..%9.3f]   composition %9.3f ms [%9.3f ..%9.3f]   fused / composition %.3f   acc %.3f" % (
        (M,) + f + c + (f[0] / c[0], ib.acc_ratio)), flush=True)
    ts = []
    for rep in range(5):
        ib._handle().set_theta(theta0)
        ib.t, ib.n_rejuvenations, ib.ess = 0, 0, float(M)
        t0 = time.perf_counter()
        smc.smc2(ib, y)
        smc.smc2_run(ib, y, 2, T, window=16, verbose=False)
        if rep >= 2:
            ts.append((time.perf_counter() - t0) * 1e6 / T)
    o = med(ts)
    print("online     M = %7d   smc2_run(ibis, window 16) %9.2f us/observation [%9.2f ..%9.2f]   rejuvenations %d" % ((M,) + o + (ib.n_rejuvenations,)), flush=True)
    ib.close()

ts = []
for rep in range(3):
    s = smc.SMC(1024, 512, mod, prior, CHAIN, 0.5, seed=3, theta_map=tmap)
    t0 = time.perf_counter()
    smc.smc2(s, y)
    smc.smc2_run(s, y, 2, T, window=16, verbose=False, out=io.StringIO())
    if rep >= 1:
        ts.append((time.perf_counter() - t0) * 1e6 / T)
    s.backend.close()
print("online     SMC(1024, 512)  smc2_run(window 16)       %9.2f us/observation [%9.2f ..%9.2f]   (particle filters inside: context)" % med(ts), flush=True)
