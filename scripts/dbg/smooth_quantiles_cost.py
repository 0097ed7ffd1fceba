"""What the quantiles of the smoothed state cost.  Writes profiles/smooth_quantiles_cost.log (and prints it).  Nothing
here is a pass condition.
  shapes   512 x 1024, 1 x 8192 and 1 x (SMOOTH_Q_LDS_MAX + 1) (filters x particles: many staged clouds, the largest staged cloud,
           the first cloud that is read from global memory in every pass), T = 200, LG1D and UCSV3D, one process, one session
  timed    smc_smooth_quantiles, three levels (0.25, 0.5, 0.75) of the last state coordinate, moments on, no weights copied
  (a)      smc_smooth on the same record, the same outputs: what the call cost before.  Interleaved with the timed call (smooth,
           quantiles, ... REPS times after one warm-up of each); device events on the handle's stream (smc_last_elapsed_ms: the
           whole backward pass, with k_smooth_quantiles inside it for the timed call); medians, their difference and their ratio
  (b)      what a user did before: smc_smooth with ws copied back, smc_history_get of every step, and a sort on the host (numpy:
           argsort of the states, the running sum of the weights in that order, the first entry above p times the total) - a host
           clock around all of it (every copy synchronises), once, against the host clock around the timed call
  bytes    the kernel's least traffic, 16 N bytes per (step, filter) in each of its two passes over global memory when the cloud
           is staged, and in each of its up to 8 select passes more when it is not"""
import os
import sys
import time

ROOT = os.environ.get("SMC_ROOT") or os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, ROOT)
LOG = os.path.join(ROOT, "profiles", "smooth_quantiles_cost.log")
T, REPS = 200, 5
P = [0.25, 0.5, 0.75]
ROWS = {1: [0.5, 1.0, 0.9, 0.8, 0.0, 1.0], 3: [0.2, 0.2, 0.0, -1.0, -2.0]}
NAMES = {1: "LG1D", 3: "UCSV3D"}


def record(L, np, model, nth, n):
    _, y = L.simulate(model, ROWS[model], T, 1998)
    h = L.Handle(model, nth, n, seed=3)
    h.set_params(np.tile(ROWS[model], (nth, 1)))
    h.history_begin(T)
    h.init(float(y[0]))
    for t in range(1, T):
        h.step(float(y[t]))
    return h


def by_hand(h, np, comp):
    """the band as a user formed it before: every weight and cloud to the host, a sort there"""
    ws = h.smooth(weights=True, moments=False)[0]                        # [T][n_theta][n]
    x = np.array([h.history_get(t)[0][comp] for t in range(T)])          # [T][n_theta][n]
    order = np.argsort(x, axis=-1, kind="stable")
    cw = np.cumsum(np.take_along_axis(ws, order, axis=-1), axis=-1)
    xs = np.take_along_axis(x, order, axis=-1)
    out = np.empty(ws.shape[:2] + (len(P),))
    for j, p in enumerate(P):
        k = np.argmax(cw > p * cw[..., -1:], axis=-1)
        out[..., j] = np.take_along_axis(xs, k[..., None], axis=-1)[..., 0]
    return out


def main():
    import numpy as np
    from sequential_monte_carlo_amd import _lib as L
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    lds_max = L.smooth_quantiles_constants()[1]
    for model in (1, 3):
        for nth, n in ((512, 1024), (1, 8192), (1, lds_max + 1)):
            h = record(L, np, model, nth, n)
            comp = h.d - 1
            ms = {"smooth": [], "quantiles": []}
            wall = []
            for rep in range(REPS + 1):                                  # (the first of each is the warm-up)
                h.smooth(weights=False, moments=True)
                ms["smooth"].append(h.elapsed_ms())
                t0 = time.perf_counter()
                q = h.smooth(weights=False, moments=True, quantiles=(comp, P))[-1]
                wall.append((time.perf_counter() - t0) * 1e3)
                ms["quantiles"].append(h.elapsed_ms())
            a, b = float(np.median(ms["smooth"][1:])), float(np.median(ms["quantiles"][1:]))
            spread = max(ms["smooth"][1:]) - min(ms["smooth"][1:])
            passes = 2 if n <= lds_max else 10
            say("%-6s %3d x %-5d T %d: smc_smooth %9.3f ms (spread %.3f), smc_smooth_quantiles %9.3f ms, difference %+8.3f ms, ratio %.4f; "
                "least traffic %.1f MB" % (NAMES[model], nth, n, T, a, spread, b, b - a, b / a, passes * 16.0 * n * nth * T / 1e6))
            t0 = time.perf_counter()
            hand = by_hand(h, np, comp)
            t_hand = (time.perf_counter() - t0) * 1e3
            close = float(np.mean(np.abs(hand - q) <= 1e-9 * (1 + np.abs(q))))
            say("%-6s %3d x %-5d T %d: by hand (weights and clouds to the host, numpy sort) %10.1f ms on the host clock, the call %9.1f ms: "
                "%.1f times; %.4f of the entries agree" % (NAMES[model], nth, n, T, t_hand, float(np.median(wall[1:])),
                                                             t_hand / float(np.median(wall[1:])), close))
            h.close()
    with open(LOG, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
