"""What the exact Kalman side costs for two-state rows next to scalar rows -> profiles/ibis2_cost.log.
M in {512, 2^16, 2^20} parameter particles, T = 200, chain 3, one parameter in both samplers (scalar: theta = A of the LG1D row;
two-state: theta = Q11 of the Hodrick-Prescott row), the same session, the same process.  Host clock around calls that end in a
device synchronise, ms per call, the median of REPS repetitions after WARM warm-up ones, scalar and two-state alternating:
  filter      smc_ibis_filter over y[0:200): 200 Kalman steps per particle in one launch (k_ibis_window<Lg1Row, ..> / <Lg2Row, ..>,
              no records)
  rejuvenate  smc_ibis_rejuvenate over y[0:200), chain 3: 600 Kalman steps per particle in one launch
  smooth      smc_kalman_smooth / smc_kalman2_smooth of n = M rows over y[0:200): the call allocates, copies the rows in and
              xs, Ps [T][n](x 2, x 3) out, so at large n it is the copies that are timed
Nothing here is a pass condition.  `--resources` (needs hipcc, no GPU): registers, scratch and occupancy of the IBIS kernels of
smc_ibis.hip for both kinds of row, and of the stand-alone two-state and scalar Kalman kernels.
usage: python scripts/dbg/ibis2_cost.py [--log FILE]"""
import os
import re
import subprocess
import sys
import tempfile
import time

HERE = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, HERE)
T, CHAIN, WARM, REPS = 200, 3, 2, 5
SIZES = (512, 1 << 16, 1 << 20)


def resources():
    csrc = os.path.join(HERE, "sequential_monte_carlo_amd", "csrc")
    out = ["kernel resource use (hipcc -Rpass-analysis=kernel-resource-usage, gfx950):"]
    for src, pat in (("smc_ibis.hip", r"k_ibis_(init|reset|window|rejuvenate|permute)<"), ("smc_kalman2.hip", r"k_kalman"), ("smc_util.hip", r"k_kalman")):
        with tempfile.TemporaryDirectory() as tmp:
            err = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math", "-fPIC",
                                  "-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.path.join(tmp, "a.o"), src],
                                 cwd=csrc, capture_output=True, text=True).stderr
        rows, name = {}, None
        for line in err.splitlines():
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                name = m.group(1)
                rows[name] = {}
            for key in ("TotalSGPRs", "VGPRs", "SGPRs Spill", "VGPRs Spill", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]"):
                m = re.search(r"remark:\s+" + re.escape(key) + r": (\d+)", line)
                if m and name:
                    rows[name][key] = int(m.group(1))
        for name, row in rows.items():
            dem = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip() or name
            short = re.sub(r"\(smc::IbisView.*|\(double const\*.*", "", dem).replace("void smc::", "").replace("smc::", "")
            if re.search(pat, short):
                out.append("  %-52s VGPRs %3d  SGPRs %3d  scratch %3d B/lane  VGPR spills %d  SGPR spills %3d  occupancy %d waves/SIMD" % (
                    short, row["VGPRs"], row["TotalSGPRs"], row["ScratchSize [bytes/lane]"], row["VGPRs Spill"], row["SGPRs Spill"],
                    row["Occupancy [waves/SIMD]"]))
    return out


def main():
    import numpy as np
    import sequential_monte_carlo_amd as smc
    from sequential_monte_carlo_amd import _lib as L
    log = sys.argv[sys.argv.index("--log") + 1] if "--log" in sys.argv else os.path.join(HERE, "profiles", "ibis2_cost.log")
    rng = np.random.default_rng(3)
    y = 0.5 * np.cumsum(rng.normal(size=T)) + rng.normal(size=T)
    hp = np.array(smc.hodrick_prescott(lam=1600, y=y).raw())
    hp[6] = 0.0
    kinds = {
        "scalar": (L.MODEL_LG1D, smc.ThetaMap(L.MODEL_LG1D, [0, -1, -1, -1, -1, -1], [0.0, 1.0, 0.9, 0.8, 0.0, 1.0]),
                   smc.product_distribution([smc.TruncatedNormal(0, 1, -1, 1)])),
        "two-state": (L.MODEL_LG2D, smc.ThetaMap(L.MODEL_LG2D, [-1] * 6 + [0] + [-1] * 8, hp), smc.product_distribution([smc.Uniform(0.0, 0.6)])),
    }
    scales = 0.5 * np.arange(CHAIN, 0, -1)
    med = lambda v: sorted(v)[len(v) // 2]
    lines = ["# scripts/dbg/ibis2_cost.py: T = %d, chain %d, one parameter; one MI355X, one process; ms per call, host clock around calls that end" % (T, CHAIN),
             "# in a synchronise; median [min .. max] of %d repetitions after %d warm-up, scalar and two-state alternating.  ratio = two-state / scalar" % (REPS, WARM)]
    for M in SIZES:
        hs, ts, rows = {}, {}, {}
        for kind, (row_id, tmap, prior) in kinds.items():
            theta = np.ascontiguousarray(prior.rand_many(np.random.default_rng(3), M), dtype=np.float64)
            fam, par = prior.spec()
            h = L.IbisHandle(M, 1, np.atleast_1d(fam), np.atleast_2d(par), tmap.raw_from, tmap.raw_const, seed=3, row_id=row_id)
            h.set_theta(theta)
            hs[kind] = (h, L.host_rw_factor(theta)[0])
            rows[kind] = tmap.rows(theta)
            for c in ("filter", "rejuvenate", "smooth"):
                ts[kind, c] = []
        for rep in range(WARM + REPS):
            for kind, (h, chol) in hs.items():
                t0 = time.perf_counter()
                h.filter(y)
                t1 = time.perf_counter()
                h.rejuvenate(y, 1.0, chol, scales * scales, 99 + rep, want_moved=False)
                t2 = time.perf_counter()
                if rep >= WARM:
                    ts[kind, "filter"].append((t1 - t0) * 1e3)
                    ts[kind, "rejuvenate"].append((t2 - t1) * 1e3)
        for h, _ in hs.values():
            h.close()
        for rep in range(1 + 3):
            for kind in kinds:
                t0 = time.perf_counter()
                xs, Ps = (L.kalman_smooth if kind == "scalar" else L.kalman2_smooth)(rows[kind], y)
                t1 = time.perf_counter()
                del xs, Ps
                if rep >= 1:
                    ts[kind, "smooth"].append((t1 - t0) * 1e3)
        for c in ("filter", "rejuvenate", "smooth"):
            a, b = ts["scalar", c], ts["two-state", c]
            lines.append("M = %7d %-10s scalar %10.4f [%10.4f ..%10.4f]   two-state %10.4f [%10.4f ..%10.4f]   ratio %.2f" % (
                M, c, med(a), min(a), max(a), med(b), min(b), max(b), med(b) / med(a)))
        print("\n".join(lines[-3:]), flush=True)
    with open(log, "a") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    if "--resources" in sys.argv:
        print("\n".join(resources()))
    else:
        main()
