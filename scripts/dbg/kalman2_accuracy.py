"""How close the two-state Kalman step (csrc/smc_spec.h kalman2_step, through its host twin smc_host_kalman2_steps) is to the
recursion of src/kalman_filter.jl:3-27 in extended precision (tests/kalman2_reference.py) -> profiles/kalman2_accuracy.log.
No GPU.  The cases and the four figures are those of tests/test_kalman2_host.py (a), which asserts 16 x the maxima logged here:
  hp   hodrick_prescott, lam = 1600, T = 200, init_cov 1e3 and 1e6: the first updates cancel values of the size of init_cov to ~1
  pd   twenty random rows with |eig A| < 1 and positive-definite Q, Sigma0, T = 50
each with predict_first = 0 and 1.  usage: python scripts/dbg/kalman2_accuracy.py [--log FILE]"""
import os
import sys

HERE = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "tests"))


def main():
    import numpy as np
    import kalman2_reference as k2
    from sequential_monte_carlo_amd import _lib as L
    log = sys.argv[sys.argv.index("--log") + 1] if "--log" in sys.argv else os.path.join(HERE, "profiles", "kalman2_accuracy.log")
    lines = ["# scripts/dbg/kalman2_accuracy.py: smc_host_kalman2_steps against numpy longdouble (eps %.3g); maxima over the cases of a group" % np.finfo(np.longdouble).eps,
             "# and both predict_first values.  |d logZ| / |logZ|, max |d xf|, max |d Sf|, max |d Sf| / max |Sf| of the record"]
    for g, v in k2.measure_accuracy(L.host_kalman2_steps).items():
        lines.append("%-18s logZ rel %.3e   xf abs %.3e   Sf abs %.3e   Sf rel %.3e" % ((g,) + v))
    print("\n".join(lines))
    with open(log, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
