"""What missing observations cost on the exact-Kalman side (IBIS(..., missing=True)) -> profiles/ibis_missing_cost.log.
The sizes of profiles/ibis_cost.log: M in {512, 2^16, 2^20} parameter particles, T = 200, chain 3, the README prior.  Calls on a
handle, host clock around calls that end in a device synchronise, ms per call:
  filter      smc_ibis_filter over y[0:200): k_ibis_window without records, 200 steps in one launch
  windows     13 x (smc_ibis_window of 16 steps, the last of 8, + smc_ibis_commit): k_ibis_window with records
  rejuvenate  smc_ibis_rejuvenate over y[0:200), chain 3: k_ibis_rejuvenate<Lg1Row, 3, MISS>, 600 Kalman steps per particle
  series      u  unflagged handle, no NaN      f  flagged handle, no NaN (must launch the kernels of u)
              g  flagged handle, every tenth observation NaN (the MISS twins)
  layout      RUNS fresh processes per library, alternating (parent, new, parent, ...), one session; inside a process the series
              alternate u, f, g per repetition (2 warm-up repetitions, 7 timed; the median is kept).  The parent library has no
              flag: its processes measure u alone, with the parent's Python package (SMC_ROOT).
  usage       SMC_PARENT_ROOT=<a built checkout of the parent commit> python scripts/dbg/ibis_missing_cost.py [--log FILE]
              (without SMC_PARENT_ROOT: the new library alone)
Nothing here is a pass condition: the log states the spread it saw.
`--resources` (needs hipcc, no GPU): registers, scratch and occupancy of the MISS twins beside their MISS = false kernels."""
import json
import os
import re
import subprocess
import sys
import tempfile
import time

HERE = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
ROOT = os.environ.get("SMC_ROOT") or HERE
sys.path.insert(0, ROOT)
T, CHAIN, EVERY, RUNS, WARM, REPS = 200, 3, 10, 3, 2, 7
SIZES = (512, 1 << 16, 1 << 20)
CALLS = ("filter", "windows", "rejuvenate")


def resources(out):
    csrc = os.path.join(HERE, "sequential_monte_carlo_amd", "csrc")
    out.append("kernel resource use (hipcc -Rpass-analysis=kernel-resource-usage, gfx950); <.., true> is the MISS twin:")
    for src in ("smc_ibis.hip", "smc_util.hip"):
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
            if not re.search(r"k_(ibis_window|ibis_rejuvenate|ibis_rts_forward|ibis_rts_paths|kalman)", name):
                continue
            dem = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip() or name
            short = re.sub(r"\(.*", "", dem).replace("void smc::", "").replace("smc::", "")
            # scalar rows (the only kind with a MISS twin), and of the rejuvenation the README prior's D = 3
            if "Lg2Row" not in short and not re.search(r"k_ibis_rejuvenate<Lg1Row, [124-8],", short):
                out.append("  %-44s VGPRs %3d  SGPRs %3d  scratch %3d B/lane  VGPR spills %d  SGPR spills %3d  occupancy %d waves/SIMD" % (
                    short, row["VGPRs"], row["TotalSGPRs"], row["ScratchSize [bytes/lane]"], row["VGPRs Spill"], row["SGPRs Spill"],
                    row["Occupancy [waves/SIMD]"]))


def worker():
    import numpy as np
    import sequential_monte_carlo_amd as smc
    from sequential_monte_carlo_amd import _lib as L
    flagged = hasattr(L.IbisHandle, "set_flags")
    _, y = smc.simulate(smc.UnivariateLinearGaussian(A=0.5, B=1.0, Q=0.9, R=0.8), T, seed=1998)
    yg = np.array(y)
    yg[EVERY - 1::EVERY] = np.nan
    prior = smc.product_distribution([smc.TruncatedNormal(0, 1, -1, 1), smc.LogNormal(0, 1), smc.LogNormal(0, 1)])
    tmap = smc.ThetaMap(1, [0, -1, 1, 2, -1, -1], [0.0, 1.0, 0.0, 0.0, 0.0, 1.0])
    fam, par = prior.spec()
    series = [("u", 0, y)] + ([("f", L.FLAG_NAN_MISSING, y), ("g", L.FLAG_NAN_MISSING, yg)] if flagged else [])
    scales = 0.5 * np.arange(CHAIN, 0, -1)
    out = {}
    for M in SIZES:
        theta = np.ascontiguousarray(prior.rand_many(np.random.default_rng(3), M), dtype=np.float64)
        chol, _ = L.host_rw_factor(theta)
        hs = {}
        for key, flags, _ in series:
            hs[key] = L.IbisHandle(M, 3, np.atleast_1d(fam), np.atleast_2d(par), tmap.raw_from, tmap.raw_const, seed=3)
            hs[key].set_theta(theta)
            if flags:
                hs[key].set_flags(flags)
        ts = {(key, c): [] for key, _, _ in series for c in CALLS}
        for rep in range(WARM + REPS):
            for key, _, ys in series:
                h = hs[key]
                t0 = time.perf_counter()
                h.filter(ys)
                t1 = time.perf_counter()
                h.set_theta(theta)
                t2 = time.perf_counter()
                for lo in range(0, T, 16):
                    k = min(16, T - lo)
                    h.window(ys[lo:lo + k])
                    h.commit(k)
                t3 = time.perf_counter()
                h.rejuvenate(ys, 1.0, chol, scales, 99 + rep, want_moved=False)
                t4 = time.perf_counter()
                h.set_theta(theta)
                if rep >= WARM:
                    ts[key, "filter"].append((t1 - t0) * 1e3)
                    ts[key, "windows"].append((t3 - t2) * 1e3)
                    ts[key, "rejuvenate"].append((t4 - t3) * 1e3)
        for (key, c), v in ts.items():
            out["%d %s %s" % (M, c, key)] = sorted(v)[len(v) // 2]
        for h in hs.values():
            h.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    log = sys.argv[sys.argv.index("--log") + 1] if "--log" in sys.argv else os.path.join(HERE, "profiles", "ibis_missing_cost.log")
    roots = {"new": HERE}
    if os.environ.get("SMC_PARENT_ROOT"):
        roots["parent"] = os.environ["SMC_PARENT_ROOT"]
    order = [k for k in ("parent", "new") if k in roots]
    res = {k: [] for k in order}
    for i in range(RUNS):
        for k in order:
            env = dict(os.environ, SMC_ROOT=roots[k])
            env.pop("SMC_LIB", None)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker"], env=env, capture_output=True, text=True, timeout=280)
            if p.returncode != 0:   # whatever ended a process: nothing more is started
                sys.exit("worker %s run %d ended with %d\n%s\n%s" % (k, i, p.returncode, p.stdout[-2000:], p.stderr[-2000:]))
            res[k].append(json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
            print(k, i, "ok", flush=True)
    med = lambda v: sorted(v)[len(v) // 2]
    fmt = lambda v: "%9.4f [%9.4f ..%9.4f]" % (med(v), min(v), max(v))
    lines = ["# scripts/dbg/ibis_missing_cost.py: T = %d, chain %d, README prior; one MI355X, one session; ms per call, host clock around calls" % (T, CHAIN),
             "# that end in a synchronise; per process the median of %d repetitions (u, f, g alternating) after %d warm-up; %d fresh processes per" % (REPS, WARM, RUNS),
             "# library, alternating (parent, new, ...): median [min .. max] over the processes.  u unflagged, f flagged without a NaN,",
             "# g flagged with every %dth observation NaN.  filter: 200 steps, one launch; windows: 13 launches with records + commits;" % EVERY,
             "# rejuvenate: chain %d over 200 observations, one launch" % CHAIN]
    for M in SIZES:
        for c in CALLS:
            col = lambda k, s: [r["%d %s %s" % (M, c, s)] for r in res[k]]
            u, f, g = col("new", "u"), col("new", "f"), col("new", "g")
            line = "M = %7d %-10s u %s  f %s  g %s  | f - u %+.4f (%+.2f %%)  g - u %+.4f (%+.2f %%)" % (
                M, c, fmt(u), fmt(f), fmt(g), med(f) - med(u), 100 * (med(f) - med(u)) / med(u), med(g) - med(u), 100 * (med(g) - med(u)) / med(u))
            if "parent" in res:
                p = col("parent", "u")
                line += "  | parent u %s  new u - parent u %+.4f (%+.2f %%), spread of parent u %.4f" % (
                    fmt(p), med(u) - med(p), 100 * (med(u) - med(p)) / med(p), max(p) - min(p))
            lines.append(line)
    print("\n".join(lines), flush=True)
    with open(log, "a") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    if "--resources" in sys.argv:
        rows = []
        resources(rows)
        print("\n".join(rows))
    elif "--worker" in sys.argv:
        worker()
    else:
        main()
