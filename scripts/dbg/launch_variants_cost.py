"""What the host-side choice of a kernel variant costs: the library of the parent commit against this one's.  Appends to
profiles/launch_variants_refactor.log (and prints).  Nothing here is a pass condition.
  usage    SMC_LIB_PARENT=<the parent's libsmchip.so> python scripts/dbg/launch_variants_cost.py
           (the new library: SMC_LIB_NEW, or the tree's)
  rows     a. wall clock per call of a loop of 2000 smc_step calls, one LG1D filter of 1024 particles (the by-value path: host
              dispatch is the largest share there)
           b. the same on a handle with FLAG_NAN_MISSING, every tenth observation NaN
           c. the same on a guided (PROP_OPTIMAL) handle          d. the same on a conditional handle
           e. smc_log_likelihood, device events on the handle's stream, second of two calls, LG1D 1 x 2^20, T = 1000
           f. the same, 512 x 1024, T = 200 (the LDS-resident kernel)
  layout   5 fresh processes per library, alternating (parent, new, parent, ...), one session
  rule     per row: median(new) - median(parent) <= max(parent) - min(parent)
  LAUNCH_VARIANTS_LOG overrides where the log goes."""
import json
import os
import subprocess
import sys
import time

ROOT = os.environ.get("SMC_ROOT") or os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, ROOT)
LOG = os.path.join(ROOT, "profiles", "launch_variants_refactor.log")
RAW = [0.5, 1.0, 0.9, 0.8, 0.0, 1.0]
STEPS, WARM, EVERY, RUNS = 2000, 200, 10, 5
ROWS = (("a", "smc_step x 2000, LG1D 1 x 1024 (by value)", "us per call"),
        ("b", "... FLAG_NAN_MISSING, every 10th NaN", "us per call"),
        ("c", "... guided (PROP_OPTIMAL)", "us per call"),
        ("d", "... conditional", "us per call"),
        ("e", "smc_log_likelihood LG1D 1 x 1048576 T 1000", "ms"),
        ("f", "smc_log_likelihood LG1D 512 x 1024 T 200 (resident)", "ms"))


def worker():
    import ctypes as C
    import numpy as np
    from sequential_monte_carlo_amd import _lib as L
    out = {}
    _, y = L.simulate(L.MODEL_LG1D, RAW, WARM + STEPS + 1, 1998)
    yg = np.array(y)
    yg[EVERY - 1::EVERY] = np.nan
    lm, ess = (C.c_double * 1)(), (C.c_double * 1)()
    step = L.lib().smc_step
    for key, flags, ys in (("a", 0, y), ("b", L.FLAG_NAN_MISSING, yg), ("c", 0, y), ("d", L.FLAG_CONDITIONAL, y)):
        h = L.Handle(L.MODEL_LG1D, 1, 1024, seed=3, flags=flags)
        h.set_params(np.array(RAW).reshape(1, -1))
        if key == "c":
            h.set_proposal(L.PROP_OPTIMAL)
        if key == "d":
            h.set_reference(np.zeros((len(ys), 1, 1)))
        h.init(float(ys[0]))
        vals = [float(v) for v in ys[1:]]
        for v in vals[:WARM]:
            L.check(step(h._h, v, lm, ess))
        t0 = time.perf_counter()
        rc = 0
        for v in vals[WARM:]:
            rc |= step(h._h, v, lm, ess)
        out[key] = (time.perf_counter() - t0) / STEPS * 1e6
        L.check(rc)
        h.close()
    for key, nth, n, T in (("e", 1, 1 << 20, 1000), ("f", 512, 1024, 200)):
        h = L.Handle(L.MODEL_LG1D, nth, n, seed=3)
        h.set_params(np.tile(RAW, (nth, 1)))
        for _ in range(2):
            h.log_likelihood(y[:T])
        out[key] = h.elapsed_ms()
        h.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    libs = {"parent": os.environ["SMC_LIB_PARENT"],
            "new": os.environ.get("SMC_LIB_NEW") or os.path.join(ROOT, "sequential_monte_carlo_amd", "lib", "libsmchip.so")}
    res = {k: [] for k in libs}
    for i in range(RUNS):
        for k in ("parent", "new"):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker"], env=dict(os.environ, SMC_LIB=libs[k]),
                               capture_output=True, text=True, timeout=240)
            if p.returncode != 0:   # whatever ended a process: nothing more is started
                sys.exit("worker %s run %d ended with %d\n%s\n%s" % (k, i, p.returncode, p.stdout[-2000:], p.stderr[-2000:]))
            res[k].append(json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
            print(k, i, res[k][-1], flush=True)
    med = lambda v: sorted(v)[len(v) // 2]
    lines = ["# scripts/dbg/launch_variants_cost.py: library of the parent commit against the library of this one, one MI355X, one session;",
             "# a-d wall clock per smc_step call (loop of %d after %d warm-up steps), e-f device events, second of two calls; %d fresh processes" % (STEPS, WARM, RUNS),
             "# per library, alternating (parent, new, parent, ...).  rule per row: median(new) - median(parent) <= max(parent) - min(parent)"]
    ok = True
    for key, what, unit in ROWS:
        p, n = [r[key] for r in res["parent"]], [r[key] for r in res["new"]]
        d, spread = med(n) - med(p), max(p) - min(p)
        ok = ok and d <= spread
        lines.append("%s %-52s parent %s %s  median %.4f spread %.4f | new %s  median %.4f spread %.4f | new - parent %+.4f (%+.2f %%): %s"
                     % (key, what, unit, " ".join("%.4f" % v for v in p), med(p), spread, " ".join("%.4f" % v for v in n), med(n), max(n) - min(n),
                        d, 100.0 * d / med(p), "within the parent's spread" if d <= spread else "OUTSIDE the parent's spread"))
    lines.append("# all six rows within the rule: %s" % ok)
    print("\n".join(lines), flush=True)
    with open(os.environ.get("LAUNCH_VARIANTS_LOG", LOG), "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    worker() if "--worker" in sys.argv else main()
