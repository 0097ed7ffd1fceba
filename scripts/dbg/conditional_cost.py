"""What a conditional sweep costs.  Writes profiles/conditional_cost.log (and prints it).  Nothing here is a pass condition.
  shapes   512 x 1024 (filters x particles), T = 200, and one filter of 8192 particles, T = 200, for LG1D and UCSV3D
  runs     a. what smoother(paths=1, smooth=False) does on a handle without the flag: the recorded step-by-step filter, then
              one backward-simulated path per filter
           b. one sweep of ParticleGibbs on a handle with FLAG_CONDITIONAL: the same with the reference pinned, then the gather
              of the path into the reference (smc_reference_from_paths)
  columns  filter: the sum over the T steps of smc_last_elapsed_ms - for the batch of 512 the device events around every step's
           launches on the handle's stream, for the single filter (result tickets, no events) the host's clock of every call;
           walk: the device events of smc_sample_paths; adopt: host clock of smc_reference_from_paths plus a synchronisation;
           wall: host clock of the whole sweep.  Second of two sweeps; a. and b. interleaved in one session, twice (two rows:
           the spread between them is the run-to-run spread).
  A library without the flag (SMC_LIB = the parent commit's build) runs a. alone.
  CONDITIONAL_COST_LOG overrides where the log goes.  Run under `rocprofv3 --kernel-trace --stats` (a run of its own, no counters)
  for the device time per launch of k_step_cond beside k_step."""
import os
import sys
import time

ROOT = os.environ.get("SMC_ROOT") or os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, ROOT)
LOG = os.path.join(ROOT, "profiles", "conditional_cost.log")
SHAPES = ((1, 512, 1024, 200), (3, 512, 1024, 200), (1, 1, 8192, 200), (3, 1, 8192, 200))      # (model, filters, particles, T)
ROWS = {1: [0.5, 1.0, 0.9, 0.8, 0.0, 1.0], 3: [0.2, 0.2, 0.0, -1.0, -2.0]}
NAMES = {1: "LG1D", 3: "UCSV3D"}


def sweep(h, y, seed, adopt):
    """one recorded run and one path per filter; (filter ms, walk ms, adopt ms, wall ms)"""
    t0 = time.perf_counter()
    h.reseed(seed)
    h.init(float(y[0]))
    filt = h.elapsed_ms()
    for v in y[1:]:
        h.step(float(v))
        filt += h.elapsed_ms()
    h.sample_paths(1, seed + 1, want_x=not adopt)
    walk = h.elapsed_ms()
    t1 = time.perf_counter()
    if adopt:
        h.reference_from_paths(0)
        h.synchronize()
    t2 = time.perf_counter()
    return filt, walk, (t2 - t1) * 1e3, (t2 - t0) * 1e3


def main():
    import numpy as np
    from sequential_monte_carlo_amd import _lib as L
    cond = hasattr(L, "FLAG_CONDITIONAL") and "smc_set_reference" in L.EXPORTS
    lines = ["# scripts/dbg/conditional_cost.py, one MI355X, one session; second of two sweeps, a. and b. interleaved, two rounds",
             "# a: recorded filter + one path per filter, handle without the flag   b: the same on a FLAG_CONDITIONAL handle + the gather of the path",
             "# library: %s" % ("this change" if cond else "without the flag (the parent commit): a. alone")]
    for model, nth, n, T in SHAPES:
        x, y = L.simulate(model, ROWS[model], T, 1998)
        hs = [("a", L.Handle(model, nth, n, seed=3), False)]
        if cond:
            hs.append(("b", L.Handle(model, nth, n, seed=3, flags=L.FLAG_CONDITIONAL), True))
            d = hs[1][1].d
            xref = np.repeat(np.asarray(x, dtype=np.float64).reshape(d, T).T[:, :, None], nth, axis=2)
            hs[1][1].set_reference(np.ascontiguousarray(xref))
        for _, h, _ in hs:
            h.set_params(np.tile(ROWS[model], (nth, 1)))
            h.history_begin(T)
        for rnd in range(2):
            out = {}
            for k in range(2):
                for key, h, adopt in hs:
                    out[key] = sweep(h, y, 100 + 10 * rnd + k, adopt)
            a = out["a"]
            txt = "%-6s %3d x %-5d T %3d (seg %d x %d) round %d: a filter %8.3f walk %7.3f wall %8.3f ms" % (
                NAMES[model], nth, n, T, hs[0][1].seg, hs[0][1].nseg, rnd, a[0], a[1], a[3])
            if cond:
                b = out["b"]
                txt += "   b filter %8.3f walk %7.3f adopt %6.3f wall %8.3f ms   b / a: filter %.3f  filter + walk %.3f  wall %.3f" % (
                    b[0], b[1], b[2], b[3], b[0] / a[0], (b[0] + b[1]) / (a[0] + a[1]), b[3] / a[3])
            lines.append(txt)
            print(txt, flush=True)
        for _, h, _ in hs:
            h.history_end()
            h.close()
    with open(os.environ.get("CONDITIONAL_COST_LOG", LOG), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
