"""What a guided filter costs and buys against the bootstrap filter (smc_set_proposal, OPTIMAL), in one process and session.
Shapes: LG 2^20 particles x 1000 steps (k_step), LG 512 filters x 1024 (LDS-resident), UCSV 512 x 1024 and 512 x 8192 (300 steps),
and the density-tempered sampler (M = 512 parameter particles, N = 256, T = 100, device PMMH).  Every filter cell: 2 warm-up calls,
then 7 timed calls (host clock around a call that ends in a synchronise); median [min .. max] in microseconds per step, and the
sample variance of logZ over the filters of the last call (a single filter: over 16 calls with different seeds).  var x time is
the figure a sampler user cares about: particles can be traded for it."""
import io
import os
import sys
import time

sys.path.insert(0, os.environ.get("SMC_ROOT") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import numpy as np
import sequential_monte_carlo_amd as smc
from sequential_monte_carlo_amd import _lib as L
from sequential_monte_carlo_amd.smc_samplers import HipBackend

LGR = [0.5, 1.0, 0.9, 0.8, 0.0, 1.0]
UCR = [0.2, 0.2, 0.0, -1.0, -2.0]


def cell(h, y):
    for _ in range(2):
        h.log_likelihood(y)
    ts = []
    for _ in range(7):
        t0 = time.perf_counter()
        z = h.log_likelihood(y)
        ts.append((time.perf_counter() - t0) * 1e6 / len(y))
    ts.sort()
    if h.n_theta == 1:
        zs = []
        for s in range(16):
            h.reseed(1000 + s)
            zs.append(h.log_likelihood(y)[0])
        z = np.array(zs)
    return ts[3], ts[0], ts[-1], float(np.var(z, ddof=1))


for name, model, raw, nth, n, T in (("LG 2^20 x 1000 (k_step)", 1, LGR, 1, 1 << 20, 1000), ("LG 512 x 1024 (resident)", 1, LGR, 512, 1024, 1000),
                                    ("UCSV 512 x 1024", 3, UCR, 512, 1024, 300), ("UCSV 512 x 8192", 3, UCR, 512, 8192, 300)):
    _, y = L.simulate(model, raw, T, 1998)
    h = L.Handle(model, nth, n, seed=3)
    h.set_params(np.tile(raw, (nth, 1)))
    rows = {}
    for label, kind in (("bootstrap", L.PROP_NONE), ("guided", L.PROP_OPTIMAL), ("bootstrap", L.PROP_NONE), ("guided", L.PROP_OPTIMAL)):
        h.reseed(3)
        h.set_proposal(kind)
        r = cell(h, y)
        rows.setdefault(label, []).append(r)
        print("%-26s %-9s %8.2f [%8.2f ..%8.2f] us/step   var(logZ) %.4g" % ((name, label) + r), flush=True)
    tb, tg = np.mean([r[0] for r in rows["bootstrap"]]), np.mean([r[0] for r in rows["guided"]])
    vb, vg = np.mean([r[3] for r in rows["bootstrap"]]), np.mean([r[3] for r in rows["guided"]])
    print("%-26s time guided / bootstrap %.3f   var guided / bootstrap %.3f   (var x time) ratio %.3f" % (name, tg / tb, vg / vb, tg * vg / (tb * vb)), flush=True)
    h.close()

# the density-tempered sampler, device PMMH: wall time of the whole run and the variance of the inner logZ at the posterior mean
m = smc.UnivariateLinearGaussian(A=0.5, B=1.0, Q=0.9, R=0.8)
_, y = smc.simulate(m, 100, seed=1998)
prior = smc.product_distribution([smc.TruncatedNormal(0, 1, -1, 1), smc.LogNormal(0, 1), smc.LogNormal(0, 1)])
tmap = smc.ThetaMap(1, [0, -1, 1, 2, -1, -1], [0.0, 1.0, 0.0, 0.0, 0.0, 1.0])


def mod(th):
    return smc.UnivariateLinearGaussian(A=th[0], B=1.0, Q=th[1], R=th[2])


for label, prop in (("bootstrap", None), ("guided", smc.OptimalProposal()), ("bootstrap", None), ("guided", smc.OptimalProposal())):
    ts = []
    for rep in range(3):
        s = smc.SMC(256, 512, mod, prior, 2, 0.5, seed=3, backend=HipBackend(proposal=prop), theta_map=tmap)
        t0 = time.perf_counter()
        stages = smc.density_tempered(s, y, verbose=False, out=io.StringIO())
        ts.append(time.perf_counter() - t0)
        s.backend.close()
    print("dt sampler M=512 N=256 T=100 %-9s %7.1f ms [%7.1f ..%7.1f]  stages %d  mean(theta) %s" % (
        label, 1e3 * sorted(ts)[1], 1e3 * min(ts), 1e3 * max(ts), len(stages), np.round(smc.expected_parameters(s), 4)), flush=True)
