"""What the predictive checks cost.  Writes profiles/predictive_cost.log (and prints it).  Nothing here is a pass
condition; no time is fixed in advance.  One process, one session (the parent's library runs in child processes of it).
  (a)  smc_predictive against smc_smooth_quantiles on the same record: 512 x 1024, T = 200, LG1D and UCSV3D.  Device events on the
       handle's stream (smc_last_elapsed_ms), medians of REPS calls after a warm-up.
  (b)  smc_get_predictive against smc_get_moments on the current state of one filter of 2^20 particles and of 512 x 1024: both calls
       wait for their results, so the host clock around the call (median of REPS); smc_get_predictive also by device events.
  (c)  the switch: smc_get_predictive of 1 and of 64 clouds of 1024 .. 16384 particles through the one-workgroup kernel
       (SMC_PRED_SMALL_MAX = 16384) and through the launches per level (SMC_PRED_SMALL_MAX = 0), device events.
  (d)  by hand: every recorded cloud to the host (smc_history_get), the terms there with scipy.special.ndtr, numpy sums; host clock,
       once, against the host clock around smc_predictive.
  (e)  log_likelihood WITHOUT the keyword, 512 x 1024, T = 200, LG1D, device events: this tree, and with --parent DIR the tree of the
       parent commit built there (its package and library), alternating, in child processes.  Nothing it launches changed."""
import os
import subprocess
import sys
import time

ROOT = os.environ.get("SMC_ROOT") or os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, ROOT)
LOG = os.path.join(os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")), "profiles", "predictive_cost.log")
T, REPS = 200, 7
P = [0.25, 0.5, 0.75]
ROWS = {1: [0.5, 1.0, 0.9, 0.8, 0.0, 1.0], 3: [0.2, 0.2, 0.0, -1.0, -2.0]}
NAMES = {1: "LG1D", 3: "UCSV3D"}


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def loglik_only():
    """(e) in this process: whatever package SMC_ROOT names"""
    import numpy as np
    from sequential_monte_carlo_amd import _lib as L
    _, y = L.simulate(1, ROWS[1], T, 1998)
    h = L.Handle(1, 512, 1024, seed=3)
    h.set_params(np.tile(ROWS[1], (512, 1)))
    ms = []
    for _ in range(REPS + 1):
        h.log_likelihood(y)
        ms.append(h.elapsed_ms())
    h.close()
    print("LOGLIK %.4f %.4f %.4f" % (med(ms[1:]), min(ms[1:]), max(ms[1:])))


def child_loglik(root):
    env = dict(os.environ, SMC_ROOT=root)
    env.pop("SMC_LIB", None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--loglik-only"], env=env, capture_output=True, text=True, timeout=300)
    for line in out.stdout.splitlines():
        if line.startswith("LOGLIK"):
            return [float(v) for v in line.split()[1:]]
    raise RuntimeError("child failed: " + out.stdout[-500:] + out.stderr[-500:])


def record(L, np, model, nth, n, steps):
    _, y = L.simulate(model, ROWS[model], steps, 1998)
    h = L.Handle(model, nth, n, seed=3)
    h.set_params(np.tile(ROWS[model], (nth, 1)))
    h.history_begin(steps)
    h.init(float(y[0]))
    for t in range(1, steps):
        h.step(float(y[t]))
    return h, y


def by_hand(h, np, ndtr, model, raw, y):
    out = np.empty((3, T, h.n_theta))
    for t in range(T):
        x = h.history_get(t)[0]                                            # [d][n_theta][n]
        if model == 1:
            ym, s2 = raw[1] * x[0], np.full_like(x[0], raw[3])
        else:
            ym, s2 = x[0], np.exp(x[2])
        out[0, t] = ndtr((y[t] - ym) / np.sqrt(s2)).mean(axis=-1)
        out[1, t] = ym.mean(axis=-1)
        out[2, t] = s2.mean(axis=-1) + ym.var(axis=-1)
    return out


def main():
    import numpy as np
    from scipy.special import ndtr
    from sequential_monte_carlo_amd import _lib as L
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("(a), (d)  the record of 512 x 1024, T = %d" % T)
    for model in (1, 3):
        h, y = record(L, np, model, 512, 1024, T)
        ms = {"q": [], "p": []}
        wall = []
        for _ in range(REPS + 1):
            h.smooth(weights=False, moments=True, quantiles=(h.d - 1, P))
            ms["q"].append(h.elapsed_ms())
            t0 = time.perf_counter()
            rows = h.predictive_record(y)
            wall.append((time.perf_counter() - t0) * 1e3)
            ms["p"].append(h.elapsed_ms())
        a, b = med(ms["q"][1:]), med(ms["p"][1:])
        say("%-6s smc_smooth_quantiles %9.3f ms, smc_predictive %7.3f ms (min %.3f max %.3f) by device events: %.5f of it; "
            "the clouds it reads: %.1f MB" % (NAMES[model], a, b, min(ms["p"][1:]), max(ms["p"][1:]), b / a,
                                             (2 if model == 1 else 4) * 8.0 * 512 * 1024 * T / 1e6))
        t0 = time.perf_counter()
        hand = by_hand(h, np, ndtr, model, ROWS[model], y)
        t_hand = (time.perf_counter() - t0) * 1e3
        err = [float(np.max(np.abs(hand[k] - rows[k]))) for k in range(3)]
        say("%-6s by hand (clouds to the host, scipy ndtr, numpy) %9.1f ms on the host clock, smc_predictive %7.2f ms: %.0f times; "
            "largest differences %.1e %.1e %.1e" % (NAMES[model], t_hand, med(wall[1:]), t_hand / med(wall[1:]), *err))
        h.close()

    say("(b)  the current state: smc_get_predictive against smc_get_moments, host clock around the call (both wait)")
    for model in (1, 3):
        for nth, n in ((1, 1 << 20), (512, 1024)):
            h, y = record(L, np, model, nth, n, 3)
            tm, tp, ev = [], [], []
            for _ in range(REPS + 1):
                t0 = time.perf_counter()
                h.moments()
                tm.append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter()
                h.predictive(float(y[2]))
                tp.append((time.perf_counter() - t0) * 1e3)
                ev.append(h.elapsed_ms())
            say("%-6s %3d x %-7d smc_get_moments %7.3f ms, smc_get_predictive %7.3f ms on the host clock (%.3f ms by device events)" % (
                NAMES[model], nth, n, med(tm[1:]), med(tp[1:]), med(ev[1:])))
            h.close()

    say("(c)  the switch: one workgroup per cloud against the launches per level, smc_get_predictive by device events, LG1D")
    for nth in (1, 64):
        for n in (1024, 2048, 4096, 8192, 16384):
            h, y = record(L, np, 1, nth, n, 2)
            res = {}
            for name, env in (("one workgroup", "16384"), ("per level", "0")):
                os.environ["SMC_PRED_SMALL_MAX"] = env
                ev = []
                for _ in range(REPS + 1):
                    h.predictive(float(y[1]))
                    ev.append(h.elapsed_ms())
                res[name] = med(ev[1:])
            os.environ.pop("SMC_PRED_SMALL_MAX", None)
            say("%3d x %-6d one workgroup %7.4f ms, per level %7.4f ms" % (nth, n, res["one workgroup"], res["per level"]))
            h.close()

    parent = sys.argv[sys.argv.index("--parent") + 1] if "--parent" in sys.argv else None
    say("(e)  log_likelihood without the keyword, 512 x 1024, T = %d, LG1D, device events: median (min .. max) of %d calls per process" % (T, REPS))
    for rep in range(3):
        a = child_loglik(ROOT)
        say("this tree   %8.3f ms (%.3f .. %.3f)" % tuple(a))
        if parent:
            b = child_loglik(parent)
            say("the parent  %8.3f ms (%.3f .. %.3f)" % tuple(b))
    with open(LOG, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    if "--loglik-only" in sys.argv:
        loglik_only()
    else:
        main()
