"""What a missing observation costs.  Writes profiles/missing_cost.log (and prints it).  Nothing here is a pass condition.
  shapes   512 x 1024 (filters x particles) LG1D and UCSV3D, T = 200 (the LDS-resident kernel), and one LG1D filter of 2^20
           particles, T = 1000 (one launch per step)
  series   a. no gaps, handle without FLAG_NAN_MISSING     b. no gaps, flagged handle (must be the same kernels as a.)
           c. every tenth observation missing, flagged handle
  columns  device time of smc_log_likelihood (events on the handle's stream, second of two calls; a., b., c. interleaved in one
           session) in ms per series, and the per-step ratio gap : observed implied by c. against b.:
           with g = the fraction of gaps, t_c = (1 - g) t_obs + g t_gap and t_obs = t_b / T  =>  t_gap / t_obs
  MISSING_COST_LOG overrides where the log goes.  Run under `rocprofv3 --kernel-trace --stats` (a run of its own, no counters) for
  the register and scratch use of the MISS instantiations beside their ordinary twins."""
import os
import sys

ROOT = os.environ.get("SMC_ROOT") or os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, ROOT)
LOG = os.path.join(ROOT, "profiles", "missing_cost.log")
SHAPES = ((1, 512, 1024, 200), (3, 512, 1024, 200), (1, 1, 1 << 20, 1000))      # (model, filters, particles, T)
ROWS = {1: [0.5, 1.0, 0.9, 0.8, 0.0, 1.0], 3: [0.2, 0.2, 0.0, -1.0, -2.0]}
NAMES = {1: "LG1D", 3: "UCSV3D"}
EVERY = 10


def main():
    import numpy as np
    from sequential_monte_carlo_amd import _lib as L
    lines = ["# scripts/dbg/missing_cost.py, one MI355X, one session; smc_log_likelihood, device events on the handle's stream, second of two calls",
             "# a: no gaps, unflagged handle   b: no gaps, FLAG_NAN_MISSING   c: every %dth observation NaN, FLAG_NAN_MISSING" % EVERY]
    for model, nth, n, T in SHAPES:
        _, y = L.simulate(model, ROWS[model], T, 1998)
        yg = np.array(y)
        yg[EVERY - 1::EVERY] = np.nan
        g = float(np.isnan(yg).mean())
        hu = L.Handle(model, nth, n, seed=3)
        hf = L.Handle(model, nth, n, seed=3, flags=L.FLAG_NAN_MISSING)
        for h in (hu, hf):
            h.set_params(np.tile(ROWS[model], (nth, 1)))
        ms = {"a": [], "b": [], "c": []}
        for _ in range(2):
            for key, h, ys in (("a", hu, y), ("b", hf, y), ("c", hf, yg)):
                h.log_likelihood(ys)
                ms[key].append(h.elapsed_ms())
        a, b, c = ms["a"][1], ms["b"][1], ms["c"][1]
        ratio = ((c - (1.0 - g) * b) / g) / b
        lines.append("%-6s %3d x %-7d T %4d (%s): a %8.3f ms  b %8.3f ms  c %8.3f ms (first calls %.3f / %.3f / %.3f); c / b = %.3f; "
                     "per step, gap : observed = %.2f" % (NAMES[model], nth, n, T, "resident" if hu.resident and hu.nseg == 1 else "one launch per step",
                                                          a, b, c, ms["a"][0], ms["b"][0], ms["c"][0], c / b, ratio))
        print(lines[-1], flush=True)
        hu.close()
        hf.close()
    with open(os.environ.get("MISSING_COST_LOG", LOG), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
