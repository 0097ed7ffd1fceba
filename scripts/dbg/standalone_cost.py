"""Wall clock of the entry points without a handle (csrc/smc_util.hip, smc_kalman2.hip, smc_kalman_smooth): per row five warm-up
calls, then the median of 50 calls, repeated five times.  One process; the library is the tree's, or SMC_LIB's.

    python scripts/dbg/standalone_cost.py > new.txt                       # us per call, five medians per row
    SMC_LIB=/path/to/parent/libsmchip.so python scripts/dbg/standalone_cost.py > parent.txt
    python scripts/dbg/standalone_cost.py --compare parent.txt new.txt    # the table of profiles/call_scope_refactor.log

Rule of the table: median(new) - median(parent) <= max(parent) - min(parent), per row."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def rows():
    import numpy as np
    from sequential_monte_carlo_amd import _lib as L
    rng = np.random.default_rng(1)
    out = []
    for k in (10, 14, 16, 20):
        n = 1 << k
        logw = rng.normal(size=n) * 5 - 100
        w = L.normalize(logw)[1]
        out.append(("normalize 2^%d" % k, lambda logw=logw: L.normalize(logw)))
        out.append(("resample 2^%d" % k, lambda w=w: L.resample(w, seed=4, stream=2, t=9)))
    M, T = 512, 200
    y = rng.normal(size=T)
    lg = np.tile([0.5, 1.0, 0.9, 0.8, 0.0, 1.0], (M, 1))
    lg[:, 0] = rng.uniform(-0.95, 0.95, M)
    a = rng.uniform(-0.4, 0.4, size=(M, 4)) + np.array([0.5, 0.0, 0.0, 0.5])
    lg2 = np.concatenate([a, np.tile([1.0, 0.5, 1.0, 0.3, 0.5, 0.4, 0.0, 0.0, 1.0, 0.0, 1.0], (M, 1))], axis=1)
    out.append(("kalman_log_likelihood 512 x 200", lambda: L.kalman_log_likelihood(lg, y)))
    out.append(("kalman2_log_likelihood 512 x 200", lambda: L.kalman2_log_likelihood(lg2, y)))
    out.append(("kalman_smooth 512 x 200", lambda: L.kalman_smooth(lg, y)))
    out.append(("kalman2_smooth 512 x 200", lambda: L.kalman2_smooth(lg2, y)))
    xp, z = rng.normal(size=(1, 4096)), rng.normal(size=(1, 4096))
    out.append(("device_filter_steps LG1D 4096", lambda: L.device_filter_steps(L.MODEL_LG1D, lg[0], L.PROP_NONE, None, xp, z, 0.7)))
    return out


def measure():
    for name, call in rows():
        meds = []
        for _ in range(5):
            for _ in range(5):
                call()
            ts = []
            for _ in range(50):
                t0 = time.perf_counter()
                call()
                ts.append(time.perf_counter() - t0)
            meds.append(statistics.median(ts) * 1e6)
        print("%-34s | %s" % (name, " ".join("%.2f" % m for m in meds)), flush=True)


def read(path):
    table = {}
    for line in open(path):
        if "|" in line:
            name, vals = line.split("|")
            table[name.strip()] = [float(v) for v in vals.split()]
    return table


def compare(parent_path, new_path):
    parent, new = read(parent_path), read(new_path)
    ok = True
    print("# us per call: five medians of 50 calls; rule per row: median(new) - median(parent) <= max(parent) - min(parent)")
    for name, p in parent.items():
        q = new[name]
        mp, mq, spread = statistics.median(p), statistics.median(q), max(p) - min(p)
        good = mq - mp <= spread
        ok = ok and good
        print("%-34s parent %s  median %.2f spread %.2f | new %s  median %.2f | new - parent %+.2f (%+.1f %%): %s"
              % (name, " ".join("%.2f" % v for v in p), mp, spread, " ".join("%.2f" % v for v in q), mq, mq - mp, 100 * (mq - mp) / mp,
                 "within the parent's spread" if good else "SLOWER than the parent's spread allows"))
    print("# all rows within the rule: %s" % ok)


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        compare(sys.argv[2], sys.argv[3])
    else:
        measure()
