"""The Monte-Carlo standard error behind tests/test_gpu_ibis_summaries.py::test_forecast_mean_against_the_grid_posterior: the
one-step forecast mean (observation_dist, ahead = 1) of the CPU restatement of src/ibis.jl (tests/ibis_reference.py; M = 512,
chain 3, threshold 0.5, T = 100) over 16 seeds, by the exactly rounded restatement of plotting_utils.jl
(tests/ibis_summary_reference.py).  No GPU.   python scripts/dbg/ibis_forecast_se.py"""
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sequential_monte_carlo_amd as smc  # noqa: E402
import ibis_summary_reference as ref  # noqa: E402
from ibis_reference import IbisReference, LG_TRUE, Y_SEED, case_one_parameter  # noqa: E402

SEEDS = list(range(1, 17))
y = smc.simulate(smc.UnivariateLinearGaussian(**LG_TRUE), 100, seed=Y_SEED)[1]
tmap, prior, _ = case_one_parameter(smc)
grid, grid_A = ref.grid_predictive_mean(y)
est = []
for seed in SEEDS:
    r = IbisReference(512, tmap, prior, 3, 0.5, seed=seed).run(y)
    est.append(ref.summary(tmap.rows(r.theta), r.x, r.S, r.logw, 1)["y"])
    print("seed %2d  forecast mean %.6f  rejuvenations %d" % (seed, est[-1], r.n_rejuvenations), flush=True)
est = np.array(est)
print("grid forecast mean %.6f (E[A] %.6f); restatement mean %.6f, sd over seeds %.6f, SE of the mean of %d seeds %.6f" % (
    grid, grid_A, est.mean(), est.std(ddof=1), len(SEEDS), est.std(ddof=1) / np.sqrt(len(SEEDS))))
