"""What the RTS smoother of an IBIS cloud costs, in one process and session -> profiles/ibis_smoother_cost.log.
For M in {512, 2^16, 2^20} parameter particles and T = 200 observations, README prior:
  smooth        smc_ibis_smooth (out only, and with the per-particle xs, Ps stored on the device): its three kernels (forward
                filter, backward pass with the chunk records, combine) by device events on the handle's stream
                (smc_ibis_last_elapsed_ms), the second of two calls; against the time 32 T M bytes take at the HBM rate a copy
                kernel achieves on this chip (6.29 TB/s)
  paths         smc_ibis_sample_paths for Mp = 1024 and 2^16, the same way (one kernel; 40 T Mp bytes: the record written and read, the paths written)
  call          the whole call on the host clock (allocation, kernels, copies back), the second of two
  smc2_run      microseconds per observation of smc2 + smc2_run(window=16, chain 3) on the same cloud size, host clock, the
                second of two runs: what the sampler that produced the cloud paid per period
The numbers are written down, not gated.  `--resources` (needs hipcc, no GPU): registers, scratch and occupancy of the kernels."""
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.environ.get("SMC_ROOT") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
HBM_BYTES_PER_S = 6.29e12


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
        if name and len(row) == 5 and "k_ibis_rts" in name:
            short = re.sub(r"^_ZN3smc\d+", "", name)[:34]
            print("  %-36s VGPRs %3d  scratch %3d B/lane  VGPR spills %d  SGPR spills %3d  occupancy %d waves/SIMD" % (
                short, row["VGPRs"], row["ScratchSize [bytes/lane]"], row["VGPRs Spill"], row["SGPRs Spill"], row["Occupancy [waves/SIMD]"]))
            name = None


if "--resources" in sys.argv:
    resources()
    sys.exit(0)

import numpy as np
import sequential_monte_carlo_amd as smc
from sequential_monte_carlo_amd import _lib as L

T, CHAIN = 200, 3
_, y = smc.simulate(smc.UnivariateLinearGaussian(A=0.5, B=1.0, Q=0.9, R=0.8), T, seed=1998)
prior = smc.product_distribution([smc.TruncatedNormal(0, 1, -1, 1), smc.LogNormal(0, 1), smc.LogNormal(0, 1)])
tmap = smc.ThetaMap(1, [0, -1, 1, 2, -1, -1], [0.0, 1.0, 0.0, 0.0, 0.0, 1.0])


def mod(th):
    return smc.UnivariateLinearGaussian(A=th[0], B=1.0, Q=th[1], R=th[2])


def second_of_two(f):
    """(host seconds, device-event ms) of the second of two calls of f, which makes one smooth / sample_paths call on h"""
    f()
    t0 = time.perf_counter()
    h = f()
    return time.perf_counter() - t0, h.last_elapsed_ms()


print("RTS smoother of an IBIS cloud, T = %d; kernels by device events, calls and smc2_run on the host clock; the second of two" % T)
for M in (512, 1 << 16, 1 << 20):
    ib = smc.IBIS(M, mod, prior, CHAIN, 0.5, seed=3, theta_map=tmap)
    theta0 = ib.theta
    run_us = 0.0
    for _ in range(2):
        ib._handle().set_theta(theta0)
        ib.t, ib.n_rejuvenations, ib.ess = 0, 0, float(M)
        t0 = time.perf_counter()
        smc.smc2(ib, y)
        smc.smc2_run(ib, y, 2, T, window=16, verbose=False)
        run_us = (time.perf_counter() - t0) * 1e6 / T
    print("M = %7d   smc2_run        %10.2f us/observation (%d rejuvenations)" % (M, run_us, ib.n_rejuvenations), flush=True)
    h = ib._handle()
    floor_ms = 32.0 * T * M / HBM_BYTES_PER_S * 1e3
    for name, states in (("smooth", False), ("smooth + xs, Ps", True)):
        if states and M > (1 << 16):       # (the copies back would be 3.4 GB: the kernel that stores is timed at the smaller sizes)
            continue

        def call(states=states):
            h.smooth(y, states=states)
            return h
        wall, ms = second_of_two(call)
        print("M = %7d   %-15s kernels %9.3f ms = %7.3f us/observation; 32 T M bytes at 6.29 TB/s: %8.4f ms (x %.1f); call %9.3f ms" % (
            M, name, ms, ms * 1e3 / T, floor_ms, ms / floor_ms, wall * 1e3), flush=True)
    for Mp in (1024, 1 << 16):
        which = np.asarray(L.host_outer_resample(ib.logw, Mp, 12345), dtype=np.int32)

        def call(which=which):
            h.sample_paths(y, which, 777)
            return h
        wall, ms = second_of_two(call)
        pfloor = 40.0 * T * Mp / HBM_BYTES_PER_S * 1e3
        print("M = %7d   paths Mp = %5d kernel  %9.3f ms; 40 T Mp bytes at 6.29 TB/s: %8.4f ms (x %.1f); call %9.3f ms" % (
            M, Mp, ms, pfloor, ms / pfloor, wall * 1e3), flush=True)
    ib.close()
