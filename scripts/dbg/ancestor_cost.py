"""What a particle-Gibbs sweep costs with ancestor sampling beside backward simulation.  Writes profiles/ancestor_cost.log (and
prints it).  Nothing here is a pass condition.
  shapes   those of profiles/conditional_cost.log: 512 x 1024 (filters x particles) and one filter of 8192 particles, T = 200, for
           LG1D and UCSV3D
  runs     the calls of ParticleGibbs.sweep() on its handle, timed part by part:
           b. FLAG_CONDITIONAL: reseed, the recorded step-by-step filter, smc_sample_paths(M = 1) + smc_reference_from_paths
           s. FLAG_CONDITIONAL | FLAG_ANCESTOR_SAMPLING: reseed, the same filter (its record also copies the ancestor vector of every
              step), smc_ancestor_sweep
  columns  filter: the sum over the T steps of smc_last_elapsed_ms - for the batch of 512 the device events around every step's
           launches and record copies on the handle's stream, for the single filter (result tickets, no events) the host's clock of
           every call; path: the host's clock from the call that follows the last step to the end of a synchronisation of the
           handle's stream (b: the walk and the gather; s: the sweep with J, idx and kept read back, as Handle.ancestor_sweep reads
           them); wall: the host's clock of the whole sweep.  s / b of each.  Second of two sweeps; b and s interleaved in one
           process, two rounds (two rows: the spread between them is the run-to-run spread).
           filter s / b is the extra record copy: the step kernels of the two handles are the same.
  last     ParticleGibbs.sweep() itself, with and without ancestor_sampling, host clock, second of two sweeps (it also reads the path back)
  ANCESTOR_COST_LOG overrides where the log goes."""
import os
import sys
import time

ROOT = os.environ.get("SMC_ROOT") or os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, ROOT)
LOG = os.path.join(ROOT, "profiles", "ancestor_cost.log")
SHAPES = ((1, 512, 1024, 200), (3, 512, 1024, 200), (1, 1, 8192, 200), (3, 1, 8192, 200))      # (model, filters, particles, T)
ROWS = {1: [0.5, 1.0, 0.9, 0.8, 0.0, 1.0], 3: [0.2, 0.2, 0.0, -1.0, -2.0]}
NAMES = {1: "LG1D", 3: "UCSV3D"}


def sweep(h, y, seed, sampling):
    """(filter ms, path ms, wall ms) of one sweep"""
    t0 = time.perf_counter()
    h.reseed(seed)
    h.init(float(y[0]))
    filt = h.elapsed_ms()
    for v in y[1:]:
        h.step(float(v))
        filt += h.elapsed_ms()
    t1 = time.perf_counter()
    if sampling:
        h.ancestor_sweep(seed + 1)
    else:
        h.sample_paths(1, seed + 1, want_x=False)
        h.reference_from_paths(0)
    h.synchronize()
    t2 = time.perf_counter()
    return filt, (t2 - t1) * 1e3, (t2 - t0) * 1e3


def main():
    import numpy as np
    import sequential_monte_carlo_amd as smc
    from sequential_monte_carlo_amd import _lib as L
    lines = ["# scripts/dbg/ancestor_cost.py, one MI355X, one process; second of two sweeps, b and s interleaved, two rounds",
             "# b: conditional filter + smc_sample_paths(1) + smc_reference_from_paths   s: the same filter on a FLAG_ANCESTOR_SAMPLING handle + smc_ancestor_sweep"]
    for model, nth, n, T in SHAPES:
        x, y = L.simulate(model, ROWS[model], T, 1998)
        hs = [("b", L.Handle(model, nth, n, seed=3, flags=L.FLAG_CONDITIONAL), False),
              ("s", L.Handle(model, nth, n, seed=3, flags=L.FLAG_CONDITIONAL | L.FLAG_ANCESTOR_SAMPLING), True)]
        d = hs[0][1].d
        xref = np.ascontiguousarray(np.repeat(np.asarray(x, dtype=np.float64).reshape(d, T).T[:, :, None], nth, axis=2))
        for _, h, _ in hs:
            h.set_params(np.tile(ROWS[model], (nth, 1)))
            h.set_reference(xref)
            h.history_begin(T)
        for rnd in range(2):
            out = {}
            for k in range(2):
                for key, h, sampling in hs:
                    out[key] = sweep(h, y, 100 + 10 * rnd + k, sampling)
            b, s = out["b"], out["s"]
            txt = ("%-6s %3d x %-5d T %3d (seg %d x %d) round %d: b filter %8.3f path %7.3f wall %8.3f ms   s filter %8.3f path %7.3f wall %8.3f ms"
                   "   s / b: filter %.3f  path %.3f  wall %.3f" % (NAMES[model], nth, n, T, hs[0][1].seg, hs[0][1].nseg, rnd, b[0], b[1], b[2],
                                                                     s[0], s[1], s[2], s[0] / b[0], s[1] / b[1], s[2] / b[2]))
            lines.append(txt)
            print(txt, flush=True)
        for _, h, _ in hs:
            h.history_end()
            h.close()
    lines.append("# ParticleGibbs.sweep() itself (host clock, the path read back), second of two sweeps, the two chains interleaved")
    for model, nth, n, T in SHAPES:
        x, y = L.simulate(model, ROWS[model], T, 1998)
        ref = np.repeat(np.asarray(x, dtype=np.float64).reshape(-1, T).T[:, None, :], nth, axis=1)      # [T][n_theta][d]
        ref = ref[..., 0] if model == 1 else ref
        pgs = [smc.ParticleGibbs(n, y, None, reference=ref, seed=7, rows=(model, np.tile(ROWS[model], (nth, 1))), ancestor_sampling=a)
               for a in (False, True)]
        ms = [0.0, 0.0]
        for k in range(2):
            for i, pg in enumerate(pgs):
                t0 = time.perf_counter()
                pg.sweep()
                ms[i] = (time.perf_counter() - t0) * 1e3
        txt = "%-6s %3d x %-5d T %3d: sweep() backward simulation %8.3f ms   ancestor sampling %8.3f ms   ratio %.3f" % (
            NAMES[model], nth, n, T, ms[0], ms[1], ms[1] / ms[0])
        lines.append(txt)
        print(txt, flush=True)
        for pg in pgs:
            pg.close()
    with open(os.environ.get("ANCESTOR_COST_LOG", LOG), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
