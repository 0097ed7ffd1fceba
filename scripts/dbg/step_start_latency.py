"""Diagnostic (profiling build: make -C sequential_monte_carlo_amd/csrc abl): start-up latency of a k_step launch on BASELINE configs[1]
(C2: one LinearGaussian filter of 2^20 particles) - the time from the entry of a workgroup's first wave to its first pick numbers
drawn, per workgroup and as the minimum over the chip (the window in which no wave has anything to issue), next to the phase
profile of the same launch.  The report is printed by the profiling build when the handle goes.  Run as
    SMC_LIB=.../build_abl/libsmchip_abl.so SMC_DBG=1 python scripts/dbg/step_start_latency.py [repeats]
SMC_STEP_BY_VALUE=0 sends the same launches through the pointers of the view."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from sequential_monte_carlo_amd import _lib as L
raw = [0.5, 1.0, 0.9, 0.8, 0.0, 1.0]
_, y = L.simulate(1, raw, 200, 1998)
for rep in range(int(sys.argv[1]) if len(sys.argv) > 1 else 3):   # the stamps are those of the LAST launch: a few independent samples
    h = L.Handle(1, 1, 1 << 20, seed=5 + rep)
    h.set_params(raw)
    h.log_likelihood(y)
    h.log_likelihood(y)
    sys.stderr.flush()
    h.close()
