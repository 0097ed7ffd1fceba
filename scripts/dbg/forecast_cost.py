"""What a forecast costs.  Writes profiles/forecast_cost.log (and prints it).  Nothing here is a pass condition.
  shapes   512 x 1024 (filters x particles) LG1D and UCSV3D, and one filter of 2^20 particles LG1D; H = 12 horizons
  columns  device time (events on the handle's stream, second of two calls) of
             smc_forecast        three quantile levels + moments of every state row + the observation rows, per horizon
             smc_forecast_cloud  the propagation alone (no output copied: both pointers NULL), and its store rate -
                                 (d + 3) * 8 bytes per particle slot and horizon
           and, for context, smc_log_likelihood over 12 observations on the same handle geometry with the same per-step summaries
           (three levels + moments): the filter itself, twelve steps with resampling.  That call is not changed by forecasts.
  FORECAST_COST_LOG overrides where the log goes."""
import os
import sys

ROOT = os.environ.get("SMC_ROOT") or os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, ROOT)
LOG = os.path.join(ROOT, "profiles", "forecast_cost.log")
H = 12
PS = [0.25, 0.5, 0.75]
SHAPES = ((1, 512, 1024), (3, 512, 1024), (1, 1, 1 << 20))      # (model, filters, particles)
ROWS = {1: [0.5, 1.0, 0.9, 0.8, 0.0, 1.0], 3: [0.2, 0.2, 0.0, -1.0, -2.0]}
NAMES = {1: "LG1D", 3: "UCSV3D"}


def main():
    import numpy as np
    from sequential_monte_carlo_amd import _lib as L
    lines = ["# scripts/dbg/forecast_cost.py, one MI355X, one session, H = %d; device events on the handle's stream, second of two calls" % H]
    for model, nth, n in SHAPES:
        _, y = L.simulate(model, ROWS[model], H, 1998)
        h = L.Handle(model, nth, n, seed=3)
        h.set_params(np.tile(ROWS[model], (nth, 1)))
        h.set_summaries(PS, 0, moments=True)
        ll = []
        for _ in range(2):
            h.log_likelihood(y)
            ll.append(h.elapsed_ms())
        h.set_summaries()
        fc, cl = [], []
        for _ in range(2):
            h.forecast(H, 20260117, p=PS)
            fc.append(h.elapsed_ms())
        for _ in range(2):
            L.check(L.lib().smc_forecast_cloud(h._h, H, 20260117, None, None))
            cl.append(h.elapsed_ms())
        npad = h.nseg * h.seg
        gbs = (h.d + 3) * 8.0 * npad * nth * H / (cl[1] * 1e-3) / 1e9
        lines.append("%-6s %3d x %-7d H %d: smc_forecast %8.3f ms (first call %8.3f); smc_forecast_cloud %7.3f ms (first call %7.3f), %6.1f GB/s stored; "
                     "smc_log_likelihood over %d observations with the same summaries %8.3f ms (first call %8.3f)"
                     % (NAMES[model], nth, n, H, fc[1], fc[0], cl[1], cl[0], gbs, H, ll[1], ll[0]))
        print(lines[-1], flush=True)
        h.close()
    with open(os.environ.get("FORECAST_COST_LOG", LOG), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
